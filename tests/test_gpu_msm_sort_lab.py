"""GPU tier: the signed-digit split and the sort layout in place -- sort_scalars with biased_scalar, window_of, digit_to_bucket,
plan_windows, the counting sorts and the layout tail (scan, bucket_slots_kernel, scan) -- through g16_dev_msm_sort_lab, against a
big-int decomposition (tests/pass_cases.py: digits() checks sum_w d_w 2^(c w) = s and the digit range on its own).

The MSM tests compare sums at merged c = 9, 13, 16, 17, 20 and whatever per-window size the cost model picks, on random scalars and a
few special ones.  Here every window size the plans accept runs -- per-window c = 3 .. 16, merged c = 9 .. 20, bucket-space shards of
3 and 8 with every rank -- on scalars built from digit vectors: every digit 2^(c-1) - 1, a digit of exactly -2^(c-1) (bucket B - 1, the
only way to reach it with the sign set) at every window, alternating extremes, one non-zero digit at every position including the top
window (whose second word is the guard word), 0, 1, r - 1, (r +- 1) / 2 and 64 seeded values.  Checked: per bucket the multiset of
(point, window, sign); offsets, task_off and the heavy set by the model's rules; task_off[M] <= max_tasks and
ceil(offsets[M] / Lmax) <= max_segments, the bounds the prover sizes its buffers and its grid by."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc
import pass_cases as pc
import pymodel as pm
from helpers import ints_to_mont

pytestmark = pytest.mark.gpu

CP = {"bls12_381": pm.BLS12_381, "bn254": pm.BN254}
CURVES = list(CP)
SIZES = (1, 255, 257)
WINDOWS = {}   # (curve, merged, c) -> W, asked of the plan once


@pytest.fixture(scope="module")
def lab():
    import groth16_amd

    lib = groth16_amd.lib()
    ctxs = {}
    for curve, cid in fc.CURVE_ID.items():
        ctx = C.c_void_p()
        lib.check(lib.c.g16_ctx_create(cid, 0, C.byref(ctx)))
        ctxs[curve] = ctx
    yield lib, ctxs
    for ctx in ctxs.values():
        lib.c.g16_ctx_destroy(ctx)


@pytest.fixture
def knobs(monkeypatch):
    for name in ("G16_MSM_WINDOW", "G16_MSM_SEGMENT", "G16_MSM_AFFINE_LEVELS", "G16_MSM_REDUCE_G", "G16_SORT_CLASS_LOG"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def run(lab, curve, scalars, merged_c, shard_n=1, shard_r=0):
    from groth16_amd import binding

    lib, ctxs = lab
    r = CP[curve].r
    status, res = binding.msm_sort_lab(lib, ctxs[curve], ints_to_mont(scalars, r, 4), merged_c, shard_n, shard_r)
    lib.check(status)
    return res


def windows(lab, curve, merged, c):
    """the plan's W for this window size (the caller has set G16_MSM_WINDOW for a per-window plan)"""
    if (curve, merged, c) not in WINDOWS:
        WINDOWS[(curve, merged, c)] = run(lab, curve, [1], c if merged else 0)["W"]
    return WINDOWS[(curve, merged, c)]


def sizes(r, c, W):
    """1, 255, 257, and -- where the digit edges are more than that -- all of them"""
    pool = len(pc.digit_edge_scalars(r, c, W))
    return SIZES + ((pool,) if pool > max(SIZES) else ())


def check(res, scalars, c, merged, shard_n=1, shard_r=0, what=""):
    assert res["c"] == c and res["merged"] == int(merged) and res["M"] == res["B"] * res["groups"], (what, res["c"], res["merged"])
    W, B, lseg, M = res["W"], res["B"], res["Lmax"], res["M"]
    if not merged:
        assert B == 1 << (c - 1) and res["groups"] == W
    else:
        assert M >= -(-(1 << (c - 1)) // shard_n)
    assert res["K"] == sum(1 << (c * w + c - 1) for w in range(W))
    buckets, offsets, task_off, heavy = pc.sort_model(scalars, c, W, merged, B, res["groups"], lseg, shard_n, shard_r)
    got_off = res["offsets"].astype(np.int64)
    wrong = np.nonzero(got_off != offsets)[0]
    assert not len(wrong), "%s: offsets differ from the prefix of the model's bucket sizes first at bucket %d: %d, model %d" % (
        what, wrong[0], got_off[wrong[0]], offsets[wrong[0]])
    assert res["n_sorted"] == offsets[M] == len(res["sorted"])
    srt = res["sorted"]
    for b, want in buckets.items():
        words = [int(v) for v in srt[offsets[b]:offsets[b + 1]]]
        if merged:
            got = sorted((v & 0x3FFFFFF, (v >> 26) & 31, v >> 31) for v in words)
        else:
            got = sorted((v & 0x7FFFFFFF, b // B, v >> 31) for v in words)
        assert got == want, "%s: bucket %d holds (point, window, sign) %s, model %s" % (what, b, got, want)
    assert (res["task_off"].astype(np.int64) == task_off).all(), "%s: task_off is not the prefix of the segments each bucket touches" % what
    nh = int(res["heavy"][0])
    assert nh == len(heavy) and {int(b) for b in res["heavy"][1:1 + nh]} == heavy, "%s: heavy list %s, model %s" % (what, list(res["heavy"][:1 + nh]), sorted(heavy))
    assert task_off[M] <= res["max_tasks"], "%s: %d partial-sum slots, buffers sized for %d" % (what, task_off[M], res["max_tasks"])
    assert -(-int(offsets[M]) // lseg) <= res["max_segments"], "%s: %d entries in segments of %d, grid sized for %d segments" % (
        what, offsets[M], lseg, res["max_segments"])
    return buckets, heavy


@pytest.mark.parametrize("c", range(3, 17))
@pytest.mark.parametrize("curve", CURVES)
def test_per_window_digits_and_layout(lab, knobs, curve, c):
    knobs.setenv("G16_MSM_WINDOW", str(c))
    W = windows(lab, curve, False, c)
    r = CP[curve].r
    for n in sizes(r, c, W):
        scalars = pc.sort_scalars(r, c, W, n)
        buckets, _ = check(run(lab, curve, scalars, 0), scalars, c, False, what="per-window c = %d, n = %d" % (c, n))
        if n >= len(pc.digit_edge_scalars(r, c, W)):   # every edge is in: a digit of exactly -2^(c-1) in every window below the top two
            B = 1 << (c - 1)
            for w in range(W - 2):
                assert any(s for _, _, s in buckets[w * B + B - 1]), w


@pytest.mark.parametrize("c", range(9, 21))
@pytest.mark.parametrize("curve", CURVES)
def test_merged_digits_and_layout(lab, knobs, curve, c):
    W = windows(lab, curve, True, c)
    r = CP[curve].r
    for n in sizes(r, c, W):
        scalars = pc.sort_scalars(r, c, W, n)
        buckets, _ = check(run(lab, curve, scalars, c), scalars, c, True, what="merged c = %d, n = %d" % (c, n))
        if n >= len(pc.digit_edge_scalars(r, c, W)):
            top = (1 << (c - 1)) - 1
            assert {w for _, w, s in buckets[top] if s} >= set(range(W - 2))


@pytest.mark.parametrize("shard_n", [1, 3, 8])
@pytest.mark.parametrize("c", [13, 20])
@pytest.mark.parametrize("curve", CURVES)
def test_bucket_space_shards(lab, knobs, curve, c, shard_n):
    W = windows(lab, curve, True, c)
    scalars = pc.sort_scalars(CP[curve].r, c, W, 257)
    entries = 0
    for rank in range(shard_n):
        buckets, _ = check(run(lab, curve, scalars, c, shard_n, rank), scalars, c, True, shard_n, rank, what="merged c = %d, rank %d of %d" % (c, rank, shard_n))
        entries += sum(len(q) for q in buckets.values())
    assert entries == sum(1 for s in scalars for d in pc.digits(s, c, W) if d)   # the ranks' shares are the whole


@pytest.mark.parametrize("merged_c", [0, 13], ids=["per_window_c6", "merged_c13"])
@pytest.mark.parametrize("curve", CURVES)
def test_all_equal_scalars_make_one_heavy_bucket_per_window(lab, knobs, curve, merged_c):
    knobs.setenv("G16_MSM_SEGMENT", "8")
    c = merged_c or 6
    if not merged_c:
        knobs.setenv("G16_MSM_WINDOW", "6")
    W = windows(lab, curve, bool(merged_c), c)
    r = CP[curve].r
    s = pc.digit_edge_scalars(r, c, W)[-1]    # a seeded value
    scalars = [s] * 300
    res = run(lab, curve, scalars, merged_c)
    assert res["Lmax"] == 8
    buckets, heavy = check(res, scalars, c, bool(merged_c), what="300 equal scalars, segments of 8")
    nonzero = [d for d in pc.digits(s, c, W) if d]
    # 300 entries per window touch 38 or 39 segments: every used bucket is heavy (a merged plan puts equal |digits| into one bucket)
    assert heavy == set(buckets) and len(heavy) == (len({abs(d) for d in nonzero}) if merged_c else len(nonzero)) >= 10
