"""CPU tier: the two kernels of the ceremony checks, read from the built companion library (libg16_ceremony.so), held to the budgets of
DESIGN.md 4.9 (the figures of the first build, as ceilings / floors).  ceremony_digits128_kernel is the front of the coefficient sort:
256 lanes, seven words per lane staged in LDS, no scratch.  ceremony_first_bad_kernel reads a flag byte and at most one point per
lane: no LDS, no scratch.  The companion holds nothing else, and the prover library holds exactly the kernels it held before."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel: (vector registers incl. accumulation registers, scratch bytes, LDS bytes, waves per SIMD) as built
BUILT = {
    "ceremony_digits128_kernel": (26, 0, 7 * 256 * 4, 8),
    "ceremony_first_bad_kernel": (10, 0, 0, 8),
}
# kernels of the prover library: 163 of the proof, verify and key paths + 28 of the setup from an SRS, none gained or lost
TOTAL_PROVER = 163 + 28
# the kernels the coefficient sort and the sums borrow from it, by instantiation count
BORROWED = {"bucket_accumulate30_kernel": 8, "digits_kernel": 2, "bucket_slots_kernel": 1, "scan_block_sums_kernel": 1, "scan_block_offsets_kernel": 1,
            "scan_write_kernel": 1, "bucket_reduce_kernel<": 4, "window_reduce_kernel<": 4, "heavy_reduce_kernel<": 4, "bucket_combine_kernel<": 4,
            "subgroup_": 5, "pairing_": 4, "convert_bases30_kernel": 4}


def _scan(name):
    import kernel_occupancy

    import groth16_amd

    path = os.path.join(os.path.dirname(groth16_amd.lib().path), name)
    assert os.path.exists(path), path
    return kernel_occupancy.kernels(path)


@pytest.fixture(scope="module")
def kernels():
    return _scan("libg16_ceremony.so")


@pytest.fixture(scope="module")
def prover_kernels():
    return _scan("libg16_mi355x.so")


@pytest.mark.parametrize("kernel", sorted(BUILT))
def test_ceremony_kernel_budget(kernels, kernel):
    hit = [k for n, k in kernels.items() if n.startswith(kernel)]
    assert len(hit) == 1, (kernel, [n for n in kernels if "ceremony" in n])
    (k,) = hit
    regs, scratch, lds, waves = BUILT[kernel]
    assert k["max_flat_wg"] == 256, k
    assert k["vgpr"] + k["agpr"] <= regs, k
    assert k["scratch"] <= scratch, k
    assert k["lds"] == lds, k
    assert k["waves_per_simd"] >= waves, k


def test_digits_kernel_uses_no_scratch(kernels):
    (k,) = [k for n, k in kernels.items() if n.startswith("ceremony_digits128_kernel")]
    assert k["scratch"] == 0, k


def test_names_and_counts(kernels, prover_kernels):
    assert sorted(kernels) == sorted(BUILT), sorted(kernels)   # the companion's code object holds its two kernels and nothing else
    assert len(prover_kernels) == TOTAL_PROVER and not [n for n in prover_kernels if "ceremony" in n]
    for sub, count in BORROWED.items():
        assert len([n for n in prover_kernels if sub in n]) == count, sub


def test_companion_library_loads_and_exports():
    import groth16_amd
    from groth16_amd import binding

    cer = groth16_amd.lib().cer
    for name in binding.CEREMONY_EXPORTS:
        assert hasattr(cer, name), name
    hdr = open(os.path.join(ROOT, "include", "g16_ceremony.h")).read()
    import re

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
