"""CPU tier: the kernels of phase 1, read from the built companion library (libg16_phase1.so), held to the figures of the first build
 as ceilings / floors.  batch_scalar_mul_kernel keeps the accumulator and the live values of one addition in registers
and the table in HBM: two waves per SIMD, no scratch in any instantiation.  phase1_powers_kernel calls the out-of-line exponentiation
once per lane, hence its small stack.  The library holds nothing else; every library's inventory is tests/kernel_inventory.py's."""
import os
import re

import pytest

import kernel_inventory as inv

# kernel name prefix: (vector registers incl. accumulation registers, scratch bytes, LDS bytes, waves per SIMD, workgroup) as built
BUILT = {
    "batch_scalar_mul_kernel<Fp30<Bls12_381FqP>": (207, 0, 0, 2, 128),
    "batch_scalar_mul_kernel<Fp2p30<Bls12_381FqP>": (250, 0, 0, 2, 128),
    "batch_scalar_mul_kernel<Fp30<Bn254FqP>": (145, 0, 0, 3, 128),
    "batch_scalar_mul_kernel<Fp2p30<Bn254FqP>": (176, 0, 0, 2, 128),
    "phase1_powers_kernel<Fp<Bls12_381FrP>": (66, 64, 0, 7, 64),
    "phase1_powers_kernel<Fp<Bn254FrP>": (66, 64, 0, 7, 64),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels("libg16_phase1.so")


@pytest.mark.parametrize("kernel", sorted(BUILT))
def test_phase1_kernel_budget(kernels, kernel):
    regs, scratch, lds, waves, wg = BUILT[kernel]
    inv.check_budget(inv.one(kernels, prefix=kernel), wg, regs, scratch, lds, waves)


def test_names_and_counts(kernels):
    assert len(kernels) == len(BUILT), sorted(kernels)   # the code object holds the two kernels' six instantiations and nothing else
    for prefix in BUILT:
        inv.one(kernels, prefix=prefix)


def test_scalar_mul_kernels_use_no_scratch_at_two_waves(kernels):
    for prefix in BUILT:
        if prefix.startswith("batch_scalar_mul_kernel"):
            k = inv.one(kernels, prefix=prefix)
            assert k["scratch"] == 0 and k["waves_per_simd"] >= 2, (prefix, k)


def test_header_matches_exports():
    import groth16_amd
    from groth16_amd import binding

    ph1 = groth16_amd.lib().ph1
    for name in binding.PHASE1_EXPORTS:
        assert hasattr(ph1, name), name
    hdr = open(os.path.join(inv.ROOT, "include", "g16_phase1.h")).read()
    assert set(re.findall(r"\b(g16_[a-z0-9_]+)\s*\(", hdr)) == set(binding.PHASE1_EXPORTS)
