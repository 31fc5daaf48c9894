"""CPU tier: the kernels of the Lagrange form, read from the built companion library (libg16_lagrange.so), held to the figures of the
first build as ceilings / floors.  lagrange_twiddle_mul_kernel is phase 1's windowed task behind a twiddle read from
the power table: the registers of batch_scalar_mul_kernel, two waves per SIMD, no scratch in any instantiation.
lagrange_addsub_kernel holds two affine points, one inversion and the two chords.  lagrange_bitrev_kernel copies.  The library holds
nothing else; every library's inventory is tests/kernel_inventory.py's."""
import os
import re

import pytest

import kernel_inventory as inv

# kernel name prefix: (vector registers incl. accumulation registers, scratch bytes, LDS bytes, waves per SIMD, workgroup) as built
BUILT = {
    "lagrange_addsub_kernel<Fp30<Bls12_381FqP>": (176, 0, 0, 2, 128),
    "lagrange_addsub_kernel<Fp2p30<Bls12_381FqP>": (220, 0, 0, 2, 128),
    "lagrange_addsub_kernel<Fp30<Bn254FqP>": (128, 0, 0, 4, 128),
    "lagrange_addsub_kernel<Fp2p30<Bn254FqP>": (154, 0, 0, 3, 128),
    "lagrange_twiddle_mul_kernel<Fp30<Bls12_381FqP>": (207, 0, 0, 2, 128),
    "lagrange_twiddle_mul_kernel<Fp2p30<Bls12_381FqP>": (249, 0, 0, 2, 128),
    "lagrange_twiddle_mul_kernel<Fp30<Bn254FqP>": (145, 0, 0, 3, 128),
    "lagrange_twiddle_mul_kernel<Fp2p30<Bn254FqP>": (175, 0, 0, 2, 128),
    "lagrange_bitrev_kernel<Affine<Fp<Bls12_381FqP>": (28, 0, 0, 8, 64),
    "lagrange_bitrev_kernel<Affine<Fp2<Bls12_381FqP>": (52, 0, 0, 8, 64),
    "lagrange_bitrev_kernel<Affine<Fp<Bn254FqP>": (20, 0, 0, 8, 64),
    "lagrange_bitrev_kernel<Affine<Fp2<Bn254FqP>": (36, 0, 0, 8, 64),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels("libg16_lagrange.so")


@pytest.mark.parametrize("kernel", sorted(BUILT))
def test_lagrange_kernel_budget(kernels, kernel):
    regs, scratch, lds, waves, wg = BUILT[kernel]
    inv.check_budget(inv.one(kernels, prefix=kernel), wg, regs, scratch, lds, waves)


def test_names_and_counts(kernels):
    assert len(kernels) == len(BUILT), sorted(kernels)   # the code object holds the three kernels' twelve instantiations and nothing else
    for prefix in BUILT:
        inv.one(kernels, prefix=prefix)


def test_stage_kernels_use_no_scratch_at_two_waves(kernels):
    for prefix in BUILT:
        k = inv.one(kernels, prefix=prefix)
        assert k["scratch"] == 0 and k["waves_per_simd"] >= 2, (prefix, k)


def test_header_matches_exports():
    import groth16_amd
    from groth16_amd import binding

    lag = groth16_amd.lib().lag
    for name in binding.LAGRANGE_EXPORTS:
        assert hasattr(lag, name), name
    hdr = open(os.path.join(inv.ROOT, "include", "g16_lagrange.h")).read()
    assert set(re.findall(r"\b(g16_[a-z0-9_]+)\s*\(", hdr)) == set(binding.LAGRANGE_EXPORTS)
