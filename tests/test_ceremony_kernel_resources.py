"""CPU tier: the two kernels of the ceremony checks, read from the built companion library (libg16_ceremony.so), held to the budgets of
DESIGN.md 4.9 (the figures of the first build, as ceilings / floors).  ceremony_digits128_kernel is the front of the coefficient sort:
256 lanes, seven words per lane staged in LDS, no scratch.  ceremony_first_bad_kernel reads a flag byte and at most one point per
lane: no LDS, no scratch.  The companion holds nothing else, and the prover library holds no ceremony kernel (what it does hold:
tests/kernel_inventory.py)."""
import operator
import os
import re

import pytest

import kernel_inventory as inv

# kernel: (vector registers incl. accumulation registers, scratch bytes, LDS bytes, waves per SIMD) as built
BUILT = {
    "ceremony_digits128_kernel": (26, 0, 7 * 256 * 4, 8),
    "ceremony_first_bad_kernel": (10, 0, 0, 8),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels("libg16_ceremony.so")


@pytest.mark.parametrize("kernel", sorted(BUILT))
def test_ceremony_kernel_budget(kernels, kernel):
    regs, scratch, lds, waves = BUILT[kernel]
    inv.check_budget(inv.one(kernels, prefix=kernel), 256, regs, scratch, lds, waves, lds_cmp=operator.eq)


def test_digits_kernel_uses_no_scratch(kernels):
    assert inv.one(kernels, prefix="ceremony_digits128_kernel")["scratch"] == 0


def test_names_and_counts(kernels):
    assert sorted(kernels) == sorted(BUILT), sorted(kernels)   # the companion's code object holds its two kernels and nothing else
    assert not [n for n in inv.kernels() if "ceremony" in n]


def test_companion_library_loads_and_exports():
    import groth16_amd
    from groth16_amd import binding

    cer = groth16_amd.lib().cer
    for name in binding.CEREMONY_EXPORTS:
        assert hasattr(cer, name), name
    hdr = open(os.path.join(inv.ROOT, "include", "g16_ceremony.h")).read()
    assert set(re.findall(r"\b(g16_[a-z0-9_]+)\s*\(", hdr)) == set(binding.CEREMONY_EXPORTS)


def test_plan_is_half_an_fr_plan():
    """the point of the 128-bit plan: about half the windows of a plan over Fr at the same window size, and six words hold rho + K"""
    import groth16_amd as g

    for m in (1, 255, 1 << 16, 1 << 22):
        plan = g.rlc_plan(m)
        c, W = plan["window_bits"], plan["windows"]
        assert 4 <= c <= 16 and c * W <= 160
        assert c * (W - 1) < 129 <= c * W + c, plan          # the smallest W that holds 128 bits and the signed-digit carry, or one more
        assert W <= (255 + c) // c // 2 + 1, plan            # an Fr plan has ceil(256 / c) windows or more
        assert plan["chunk"] % 1024 == 0 and plan["chunk"] >= 1024
