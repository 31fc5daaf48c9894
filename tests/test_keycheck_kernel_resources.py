"""CPU tier: the kernels of the key check, read from the built companion library (libg16_keycheck.so), held to the figures of the
first build as ceilings / floors.  keycheck_rows_kernel is the gather-bound kernel of the call and the counterpart
of spmv3_kernel: it is held to that kernel's 62 registers (the instance sum is parked in its output slot; with both sums in registers
it took 76) and uses no scratch.  The library holds nothing else; every library's inventory is tests/kernel_inventory.py's."""
import pytest

import kernel_inventory as inv

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
    return inv.kernels("libg16_keycheck.so")


@pytest.mark.parametrize("kernel", sorted(BUILT))
def test_keycheck_kernel_budget(kernels, kernel):
    regs, scratch, lds, waves, wg = BUILT[kernel]
    inv.check_budget(inv.one(kernels, prefix=kernel), wg, regs, scratch, lds, waves)


def test_names_and_counts(kernels):
    assert len(kernels) == len(BUILT), sorted(kernels)   # the code object holds the four kernels' eight instantiations and nothing else
    for prefix in BUILT:
        inv.one(kernels, prefix=prefix)


def test_row_kernel_stays_within_the_prover_row_kernel(kernels):
    """against spmv3_kernel as built today, read from the prover library beside the recorded 62"""
    spmv = inv.pick(inv.kernels(), prefix="spmv3_kernel<")
    budget = max(k["vgpr"] + k["agpr"] for k in spmv.values())
    assert budget <= SPMV3_REGISTERS
    for prefix in BUILT:
        if prefix.startswith("keycheck_rows_kernel"):
            k = inv.one(kernels, prefix=prefix)
            assert k["vgpr"] + k["agpr"] <= budget and k["scratch"] == 0 and k["waves_per_simd"] == 8, (prefix, k, budget)
