"""GPU tier: the prover's MSM reductions -- heavy_reduce_kernel, bucket_combine_kernel, bucket_reduce_kernel, window_reduce_kernel and
the host fold, launched by msm_reduce / fold_windows exactly as in a proof -- on crafted partial sums (tests/reduce_cases.py), against
pymodel's group law.  Whole MSMs on random data do not reach a doubling or a cancellation inside a bucket's list of partial sums, in
the running sums over a chunk of buckets or in the trees, and the order of entries inside a bucket is not the caller's to choose; the
lab's records are.

Per curve, group, fold (per-window, merged) and buckets per reduction lane (8, 16: bit planes and host recombination live; 32: a chunk
is the whole group) two scenarios, one call each:
  combine   every crafted list in a bucket of its own; each bucket's first slot after the two combine stages is compared with the
            model's bucket sum (one test per named bucket, so a failure names kernel and collision), and the folded result
  chains    scripts for bucket_reduce_kernel's two running sums and chunks with equal / opposite sums for window_reduce_kernel's
            tree; these only show in the folded result
The collisions are asserted by the generator with the model alone (test_reduce_cases.py runs that without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc
import reduce_cases as rc
from helpers import arr_to_g1, arr_to_g2

pytestmark = pytest.mark.gpu

CONFIGS = rc.configs()
CONFIG_IDS = [rc.config_id(*cfg) for cfg in CONFIGS]
CASES = rc.combine_case_names()
RESULTS = {}   # (config, scenario) -> (first slots, folded affine point): one lab call each, shared by the tests that read it


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


def run(lab, cfg, name):
    if (cfg, name) not in RESULTS:
        from groth16_amd import binding

        lib, ctxs = lab
        curve, g2, merged, chunk = cfg
        sc = rc.scenario(*cfg, name)
        m = sc.m
        records = np.array(sc.records, dtype=np.uint32).reshape(len(sc.records), m.words)
        first, out = binding.msm_reduce_lab(lib, ctxs[curve], g2, merged, rc.C_BITS, rc.GROUPS, chunk, np.array(sc.nparts, dtype=np.uint32),
                                            records, (4 if g2 else 2) * m.cp.fq_limbs64)
        RESULTS[(cfg, name)] = (first, (arr_to_g2 if g2 else arr_to_g1)(out, m.cp)[0])
    return RESULTS[(cfg, name)]


def check_bucket(sc, first, b):
    got, want = sc.m.decode(first[b]), sc.sums[b]
    what = sc.named.get(b, "a bucket of %d partial sums" % sc.nparts[b])
    assert got == want, "bucket %d (group %d, bucket %d; %d partial sums), %s: first slot holds %s, the bucket's sum is %s" % (
        b, b // rc.B, b % rc.B, sc.nparts[b], what, "the identity" if got is None else got, "the identity" if want is None else want)


@pytest.mark.parametrize("case", CASES, ids=[c.replace(" ", "_") for c in CASES])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_combine_stage_bucket(lab, cfg, case):
    sc = rc.scenario(*cfg, "combine")
    first, _ = run(lab, cfg, "combine")
    (b,) = [k for k, v in sc.named.items() if v == case]
    check_bucket(sc, first, b)


@pytest.mark.parametrize("name", rc.SCENARIOS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_every_bucket_and_the_fold(lab, cfg, name):
    """every bucket's first slot (the unnamed random ones too), then the folded sum: bucket_reduce_kernel, window_reduce_kernel, the
    bit planes and fold_windows.  In "chains" the collisions sit in bucket_reduce_kernel's running sums and window_reduce_kernel's
    tree (reduce_cases._chains lists them)"""
    sc = rc.scenario(*cfg, name)
    first, total = run(lab, cfg, name)
    for b in range(rc.GROUPS * rc.B):
        if b not in sc.named:
            check_bucket(sc, first, b)
    bad = [sc.named[b] for b in sc.named if sc.m.decode(first[b]) != sc.sums[b]]
    assert total == sc.total, "%s: folded sum %s, model %s; collisions in this scenario: %s; named buckets with a wrong first slot: %s" % (
        name, total, sc.total, sorted(sc.seen), bad or "none")
