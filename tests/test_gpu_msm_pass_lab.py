"""GPU tier: the bucket pass's walk in place -- bucket_accumulate30_kernel as msm_bucket_pass_batch launches it, on sorted lists and
bucket histograms made by tests/pass_cases.py -- through g16_dev_msm_pass_lab, against pymodel's group law.  offsets, task_off and the
heavy list come from the library's own layout code (the tail of sort_scalars: the scan of the counts, bucket_slots_kernel, the scan of
the slot counts) and are compared with the model's too.

Whole MSMs cannot choose the order of entries inside a bucket (LDS atomics decide it) and cannot see a slot the walk never wrote (the
partial-sum buffer comes from the arena unzeroed, and may hold a previous call's right answer).  Here the order is the caller's and
the slots are pre-filled with the byte 0xA5: a slot below task_off[M] whose zz limbs still hold the fill was never written, and the 8
guard records behind the last slot must not change.

Per curve, group, fold (per-window, merged) and segment length (8, 19, 64) one lab call per job of pass_cases.JOBS, C_BITS = 6 with two
groups (64 buckets), and one call that runs four of the jobs in ONE launch: every job's records and fold must be what the job gave alone.
Every record is compared as an affine point with the model's signed sum of its share; the folded point with the model's fold."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc
import pass_cases as pc
from helpers import arr_to_g1, arr_to_g2, g1_to_arr, g2_to_arr

pytestmark = pytest.mark.gpu

G16_OK, G16_ERR_BAD_ARG = 0, 3
CONFIGS = pc.configs()
CONFIG_IDS = [pc.config_id(*cfg) for cfg in CONFIGS]
RESULTS = {}   # (config, job name) -> the lab's result for the job alone: one call each, shared by the tests that read it


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


def lab_job(job):
    cp = job.pm.m.cp
    table = (g2_to_arr if job.pm.g2 else g1_to_arr)(job.table_points(), cp)
    return {"table": table, "base_count": job.base_count, "shift": job.shift, "counts": np.array(job.counts, dtype=np.uint32),
            "sorted": np.array(job.sorted, dtype=np.uint32)}


def call(lab, cfg, jobs, **kw):
    from groth16_amd import binding

    lib, ctxs = lab
    curve, g2, merged, lseg = cfg
    m = pc.model(curve, g2).m
    args = dict(c=pc.C_BITS, groups=pc.GROUPS, G=pc.REDUCE_G, lseg=lseg, rows=pc.ROWS if merged else 1)
    args.update(kw)
    return binding.msm_pass_lab(lib, ctxs[curve], g2, merged, args["c"], args["groups"], args["G"], args["lseg"], args["rows"], jobs, m.words,
                                (4 if g2 else 2) * m.cp.fq_limbs64)


def alone(lab, cfg, name):
    if (cfg, name) not in RESULTS:
        status, res = call(lab, cfg, [lab_job(pc.job(*cfg, name))])
        assert status == G16_OK, "%s: status %d" % (name, status)
        RESULTS[(cfg, name)] = res[0]
    return RESULTS[(cfg, name)]


def show(P):
    return "the identity" if P is None else str(P)


def check(job, res):
    """a lab result against the job's model: the layout, every record (named buckets first, so that a failure names its case), the
    guards, the fold"""
    pm, m = job.pm, job.pm.m
    assert [int(x) for x in res["offsets"]] == job.offsets, "offsets are not the exclusive prefix of the counts"
    assert [int(x) for x in res["task_off"]] == job.task_off, "task_off is not the exclusive prefix of the segments each bucket touches"
    nh = int(res["heavy"][0])
    assert nh == len(job.heavy) and {int(b) for b in res["heavy"][1:1 + nh]} == job.heavy, "heavy list %s, buckets with more than %d segments: %s" % (
        list(res["heavy"][:1 + nh]), pc.HEAVY_PARTS, sorted(job.heavy))
    records = res["records"]
    n = job.task_off[pc.M]
    assert records.shape == (n + pc.GUARDS, m.words)
    names = {b: name for name, b in job.named.items()}
    zz = slice(2 * m.C * m.f.NL, 3 * m.C * m.f.NL)
    bad = []
    for b in sorted(range(pc.M), key=lambda b: (b not in names, b)):
        for k, t in enumerate(job.segs(b)):
            slot = job.task_off[b] + k
            what = "%s: bucket %d, segment %d (slot %d, entries %s as multiples of G)" % (names.get(b, "an unnamed bucket"), b, t, slot, job.shares[(b, t)])
            if (records[slot][zz] == pc.FILL_WORD).all():
                bad.append(what + ": never written, the slot still holds the fill")
                continue
            got, want = m.decode(records[slot]), pm.point(job.expected[slot])
            if got != want:
                bad.append(what + ": the record holds %s, the share's sum is %s" % (show(got), show(want)))
    assert not bad, "%s, %d of %d records wrong:\n%s" % (job.name, len(bad), n, "\n".join(bad[:6]))
    assert (records[n:] == pc.FILL_WORD).all(), "%s: a guard record behind slot %d changed" % (job.name, n)
    got = (arr_to_g2 if pm.g2 else arr_to_g1)(res["out"], m.cp)[0]
    assert got == pm.point(job.total), "%s: folded sum %s, model %s" % (job.name, show(got), show(pm.point(job.total)))


CASES = [(cfg, name) for cfg in CONFIGS for name in pc.job_names(cfg[2])]


@pytest.mark.parametrize("cfg,name", CASES, ids=["%s-%s" % (pc.config_id(*cfg), name) for cfg, name in CASES])
def test_pass_job(lab, cfg, name):
    job = pc.job(*cfg, name)
    res = alone(lab, cfg, name)
    if job.S == 0:
        assert res["records"].shape[0] == pc.GUARDS    # nothing launched, nothing written: check() looks at the guards
    check(job, res)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_four_jobs_in_one_launch(lab, cfg):
    jobs = [pc.job(*cfg, name) for name in pc.BATCH]
    status, res = call(lab, cfg, [lab_job(j) for j in jobs])
    assert status == G16_OK
    for job, got in zip(jobs, res):
        check(job, got)
        one = alone(lab, cfg, job.name)
        for key in ("records", "offsets", "task_off", "out"):
            assert (got[key] == one[key]).all(), "%s: %s differs from what the job gave alone" % (job.name, key)
        assert sorted(got["heavy"][1:1 + got["heavy"][0]]) == sorted(one["heavy"][1:1 + one["heavy"][0]])


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[3] == 19], ids=[i for c, i in zip(CONFIGS, CONFIG_IDS) if c[3] == 19])
def test_pass_lab_refusals(lab, cfg):
    """whatever would let the kernel read outside what was uploaded is refused; an index out of range after `shift` is not"""
    curve, g2, merged, lseg = cfg
    base = lab_job(pc.job(*cfg, "collisions"))
    ok = lambda **kw: call(lab, cfg, [dict(base, **{k: v for k, v in kw.items() if k in base or k in ("n_sorted", "record_cap")})],  # noqa: E731
                           **{k: v for k, v in kw.items() if k not in base and k not in ("n_sorted", "record_cap")})[0]
    counts = base["counts"].copy()
    counts[5] += 1
    assert ok(counts=counts) == G16_ERR_BAD_ARG                                   # sum(counts) != len(sorted)
    assert ok(sorted=base["sorted"][:-1]) == G16_ERR_BAD_ARG
    for bad in (7, 0, 4097, -1):
        assert ok(lseg=bad) == G16_ERR_BAD_ARG, bad
    if merged:
        srt = base["sorted"].copy()
        srt[3] |= pc.ROWS << 26
        assert ok(sorted=srt) == G16_ERR_BAD_ARG                                  # a window tag >= rows
        assert ok(rows=1) == G16_ERR_BAD_ARG                                      # (this job's tags are 0 and 1: one row is one too few)
        assert ok(rows=33) == G16_ERR_BAD_ARG
    else:
        assert ok(rows=2) == G16_ERR_BAD_ARG                                      # a per-window plan has one table
    big = np.zeros((1 << 16) + 1, dtype=np.uint32)
    cnt = np.zeros(pc.M, dtype=np.uint32)
    cnt[0] = len(big)
    assert ok(sorted=big, counts=cnt) == G16_ERR_BAD_ARG                          # more than 2^16 entries
    assert ok(c=14, groups=1, counts=np.zeros(1 << 13, dtype=np.uint32), sorted=base["sorted"][:0]) == G16_ERR_BAD_ARG   # more than 2^12 buckets
    assert call(lab, cfg, [])[0] == G16_ERR_BAD_ARG
    assert call(lab, cfg, [base] * 5)[0] == G16_ERR_BAD_ARG
    status, res = call(lab, cfg, [base])                                          # the context still works after the refusals
    assert status == G16_OK
    check(pc.job(*cfg, "collisions"), res[0])
