"""CPU tier: register / scratch budgets of the verifier kernels (verify.hip), read from the built library as
tests/test_kernel_resources.py reads the prover's.  One lane per proof: the Fq12 accumulator and the out-of-line tower products'
frames live in scratch; these bounds catch a change that multiplies it or drops the kernel below two waves per SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def kernels():
    import kernel_occupancy

    import groth16_amd

    return kernel_occupancy.kernels(groth16_amd.lib().path)


def pick(kernels, *subs):
    hit = {n: k for n, k in kernels.items() if all(s in n for s in subs)}
    assert hit, f"no kernel matches {subs}"
    return hit


@pytest.mark.parametrize("curve", ["Bls12_381FqP", "Bn254FqP"])
def test_batch_kernel_budget(kernels, curve):
    (k,) = pick(kernels, "verify_batch_kernel", curve).values()
    assert k["waves_per_simd"] >= 2, k
    assert k["lds"] == 0, k
    assert k["scratch"] <= 16 * 1024, k
    assert k["max_flat_wg"] == 64, k


def test_setup_kernels_budget(kernels):
    for sub in ("pairing_prepare_kernel", "pairing_product_kernel", "verify_window_table_kernel"):
        for name, k in pick(kernels, sub).items():
            assert k["scratch"] <= 16 * 1024, (name, k)
            assert k["lds"] == 0, (name, k)


def test_verifier_kernel_names_stay_out_of_the_prover_budgets(kernels):
    prover = ("bucket_accumulate30_kernel", "ntt30_", "digits_kernel", "build_window_tables_kernel", "spmv3_kernel")
    for name in kernels:
        if name.startswith(("verify_", "pairing_")):
            assert not any(s in name for s in prover), name
