"""CPU tier: the kernels of the key check, read from the built companion library (libg16_keycheck.so), held to the figures of the
first build as ceilings / floors.  keycheck_rows_kernel is the gather-bound kernel of the call and the counterpart
of spmv3_kernel: it is held to that kernel's 62 registers (the instance sum is parked in its output slot; with both sums in registers
it took 76) and uses no scratch.  The library holds nothing else; the other three libraries' inventories are pinned by
test_kernel_resources.py, test_ceremony_kernel_resources.py and test_phase1_kernel_resources.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SPMV3_REGISTERS = 62
# kernel name prefix: (vector registers incl. accumulation registers, scratch bytes, LDS bytes, waves per SIMD, workgroup) as built
BUILT = {
    "keycheck_rows_kernel<Fp<Bls12_381FrP>": (SPMV3_REGISTERS, 0, 0, 8, 256),
    "keycheck_rows_kernel<Fp<Bn254FrP>": (SPMV3_REGISTERS, 0, 0, 8, 256),
    "keycheck_rho_kernel<Fp<Bls12_381FrP>": (56, 0, 0, 8, 256),
    "keycheck_rho_kernel<Fp<Bn254FrP>": (56, 0, 0, 8, 256),
    "keycheck_scatter_odd_kernel<Fp<Bls12_381FrP>": (16, 0, 0, 8, 256),
    "keycheck_scatter_odd_kernel<Fp<Bn254FrP>": (16, 0, 0, 8, 256),
    "keycheck_add_kernel<Fp<Bls12_381FrP>": (48, 0, 0, 8, 256),
    "keycheck_add_kernel<Fp<Bn254FrP>": (48, 0, 0, 8, 256),
}


@pytest.fixture(scope="module")
def kernels():
    import kernel_occupancy

    import groth16_amd

    path = os.path.join(os.path.dirname(groth16_amd.lib().path), "libg16_keycheck.so")
    assert os.path.exists(path), path
    return kernel_occupancy.kernels(path)


def _one(kernels, prefix):
    hit = [k for n, k in kernels.items() if n.replace(" ", "").startswith(prefix.replace(" ", ""))]
    assert len(hit) == 1, (prefix, sorted(kernels))
    return hit[0]


@pytest.mark.parametrize("kernel", sorted(BUILT))
def test_keycheck_kernel_budget(kernels, kernel):
    k = _one(kernels, kernel)
    regs, scratch, lds, waves, wg = BUILT[kernel]
    assert k["max_flat_wg"] == wg, k
    assert k["vgpr"] + k["agpr"] <= regs, k
    assert k["scratch"] <= scratch, k
    assert k["lds"] <= lds, k
    assert k["waves_per_simd"] >= waves, k


def test_names_and_counts(kernels):
    assert len(kernels) == len(BUILT), sorted(kernels)   # the code object holds the four kernels' eight instantiations and nothing else
    for prefix in BUILT:
        _one(kernels, prefix)


def test_row_kernel_stays_within_the_prover_row_kernel(kernels):
    """against spmv3_kernel as built today, read from the prover library beside the recorded 62"""
    import kernel_occupancy

    import groth16_amd

    main = kernel_occupancy.kernels(groth16_amd.lib().path)
    spmv = [k for n, k in main.items() if n.startswith("void g16::spmv3_kernel") or n.startswith("spmv3_kernel") or "spmv3_kernel<" in n]
    assert spmv, "spmv3_kernel is not in the prover library"
    budget = max(k["vgpr"] + k["agpr"] for k in spmv)
    assert budget <= SPMV3_REGISTERS
    for prefix in BUILT:
        if prefix.startswith("keycheck_rows_kernel"):
            k = _one(kernels, prefix)
            assert k["vgpr"] + k["agpr"] <= budget and k["scratch"] == 0 and k["waves_per_simd"] == 8, (prefix, k, budget)
