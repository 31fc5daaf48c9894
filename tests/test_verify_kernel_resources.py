"""CPU tier: register / scratch budgets of the verifier kernels (verify.hip), read from the built library as
tests/test_kernel_resources.py reads the prover's.  One lane per proof: the Fq12 accumulator and the out-of-line tower products'
frames live in scratch; these bounds catch a change that multiplies it or drops the kernel below two waves per SIMD."""
import operator

import pytest

import kernel_inventory as inv
from kernel_inventory import pick


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("curve", ["Bls12_381FqP", "Bn254FqP"])
def test_batch_kernel_budget(kernels, curve):
    inv.check_budget(inv.one(kernels, "verify_batch_kernel", curve), wg=64, scratch=16 * 1024, lds=0, waves=2, lds_cmp=operator.eq)


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
