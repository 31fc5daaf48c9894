"""Shapes of the merged-plan counting sort (msm_sort.hip, sort_scalars: class partition -> sub-class partition -> LDS-resident final
level), driven through the ad-hoc MSM with window tables built on the fly (G16_MSM_API_PRECOMP=1) and a forced window size
(G16_MSM_PRECOMP_WINDOW).  The group sums depend only on which entries land in which bucket, so every case is compared bit-for-bit
with the CPU oracle's MSM.  The sizes are the smallest at which each part of the sort can go wrong:

  c = 9 / 13 / 16 / 20   a bucket set smaller than one sort class (2^8 buckets), smaller still (2^12), several classes (4), and 64
                         classes whose sub-classes are mostly empty at these n
  n = 1, 255, 257        less than a tile, one short of / one past a 256-lane row
  n = 2^13 + 1, 2^16     several partition tiles per class at small c (n * W entries over one class), more than one workgroup per class
  skew at 2^16           all scalars equal: one bucket per window holds n entries -- far beyond what the final level keeps in LDS, the
                         direct-scatter path, with every wave of the region hitting ONE LDS counter; two values; 0 / 1 / r - 1;
                         half zero (entries dropped at the first level)
  bucket-space shard     keys filtered by residue and re-indexed before the class split; the eight shares add up to the MSM
  padded regions         G16_MSM_AFFINE_LEVELS=1 keeps the histogram-matrix scatter (bucket regions padded, pre-filled with holes)
  digit edges            the scalars of the sort lab (tests/pass_cases.py::digit_edge_scalars, for all four window sizes at once): every
                         digit 2^(c-1) - 1, a digit of exactly -2^(c-1) at every window, one non-zero digit at every position; the
                         sort lab checks where their entries land, this pins the sum end to end

The oracle's result is computed once per (curve, scalar set) and shared by the window sizes."""
import numpy as np
import pytest

import pass_cases as pc
import pymodel as pm
from helpers import ints_to_mont

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
CP = {"bls12_381": pm.BLS12_381, "bn254": pm.BN254}
WINDOWS = ["9", "13", "16", "20"]
SIZES = [1, 255, 257, (1 << 13) + 1, 1 << 16]
SKEWS = ["all_equal", "two_values", "zero_one_minus_one", "half_zero"]
N_SKEW = 1 << 16


def digit_edges(curve):
    """the sort lab's edge scalars for every window size of this module, each once"""
    r = CP[curve].r
    out = []
    for c in (int(w) for w in WINDOWS):
        for s in pc.digit_edge_scalars(r, c, (r.bit_length() + c) // c):
            if s not in out:
                out.append(s)
    return out


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module", params=CURVES)
def env(request, g, orc):
    prover = g.Groth16(request.param, 0)
    yield request.param, prover
    prover.close()


@pytest.fixture(scope="module")
def cases(orc):
    """(curve, kind, n) -> (bases, scalars, oracle MSM), built on first use and never modified afterwards"""
    cache = {}

    def scalars_of(curve, kind, n):
        cp = CP[curve]
        if kind == "uniform":
            return orc.rand_fr(curve, 900 + n, n)
        if kind == "digit_edges":
            return ints_to_mont(digit_edges(curve), cp.r, 4)
        if kind == "all_equal":
            return np.repeat(orc.rand_fr(curve, 901, 1), n, axis=0)
        if kind == "two_values":
            two = orc.rand_fr(curve, 902, 2)
            return two[np.random.default_rng(3).integers(0, 2, n)]
        if kind == "zero_one_minus_one":
            three = ints_to_mont([0, 1, cp.r - 1], cp.r, 4)
            return three[np.arange(n) % 3]
        assert kind == "half_zero"
        sc = orc.rand_fr(curve, 903, n)
        sc[::2] = 0
        return sc

    def get(curve, kind, n):
        key = (curve, kind, n)
        if key not in cache:
            bases = orc.synth_bases(curve, False, 17, n)
            sc = np.ascontiguousarray(scalars_of(curve, kind, n))
            want = orc.msm(curve, False, bases, sc)
            for a in (bases, sc, want):
                a.setflags(write=False)
            cache[key] = (bases, sc, want)
        return cache[key]

    return get


@pytest.fixture
def merged(monkeypatch):
    def force(window, affine_levels="0"):
        monkeypatch.setenv("G16_MSM_API_PRECOMP", "1")
        monkeypatch.setenv("G16_MSM_PRECOMP_WINDOW", window)
        monkeypatch.setenv("G16_MSM_AFFINE_LEVELS", affine_levels)

    return force


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_sort_sizes_uniform_scalars(env, cases, merged, n, window):
    curve, prover = env
    merged(window)
    bases, sc, want = cases(curve, "uniform", n)
    assert (prover.msm(bases, sc) == want).all()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("kind", SKEWS)
def test_sort_skewed_scalars(env, cases, merged, kind, window):
    curve, prover = env
    merged(window)
    bases, sc, want = cases(curve, kind, N_SKEW)
    assert (prover.msm(bases, sc) == want).all()


@pytest.mark.parametrize("window", WINDOWS)
def test_sort_digit_edge_scalars(env, cases, merged, window):
    curve, prover = env
    merged(window)
    bases, sc, want = cases(curve, "digit_edges", len(digit_edges(curve)))
    assert (prover.msm(bases, sc) == want).all()


@pytest.mark.parametrize("window", ["13", "20"])
@pytest.mark.parametrize("kind", ["uniform", "all_equal"])
def test_sort_bucket_space_shard_of_eight(env, orc, cases, merged, kind, window):
    """every residue class of shard_n = 8 (tests/test_gpu_bucket_shard.py's entry point); an all-equal witness puts each window's
    entries on ONE rank and leaves the other seven with that window empty"""
    curve, prover = env
    merged(window)
    bases, sc, want = cases(curve, kind, N_SKEW)
    total = None
    for r in range(8):
        part = prover.msm_bucket_shard(bases, sc, r, 8, False)
        total = part if total is None else orc.group_op(curve, False, 0, total, part)
    assert (total == want).all()


@pytest.mark.parametrize("window", ["13", "20"])
def test_sort_padded_bucket_regions(env, cases, merged, window):
    curve, prover = env
    merged(window, affine_levels="1")
    bases, sc, want = cases(curve, "uniform", (1 << 13) + 1)
    assert (prover.msm(bases, sc) == want).all()
