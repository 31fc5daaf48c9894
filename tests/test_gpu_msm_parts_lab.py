"""GPU tier: the bucket-part walk in place -- bucket_parts30_kernel (msm.hip) as msm_bucket_pass_batch launches
it, on sorted lists and bucket histograms made by tests/pass_cases.py and tests/parts_cases.py -- through g16_dev_msm_parts_lab, against
pymodel's group law.  offsets, task_off, the heavy list and the task list come from the library's own layout code (msm_parts_layout:
part_count_kernel, the scans, part_place_kernel).

Per curve, group, fold (per-window, merged) and longest part (8, 19, 64) one lab call per job, C_BITS = 6 with two groups (64 buckets),
and one call that runs four of the jobs in ONE launch.  Checked (parts_cases.check): task_off is the exclusive prefix of
ceil(count / Lmax); every slot below task_off[M] was written (the slots are pre-filled with the byte 0xA5); the 8 guard records behind
the last slot are unchanged; every record is, as an affine point, the model's signed sum of exactly its part; the folded sum is the
model's.  The jobs place bucket sizes 0, 1, Lmax, Lmax + 1, 2 Lmax and 2 Lmax + 1, a bucket on the heavy list, a launch whose first wave
mixes trip counts, one whose tasks all have one length, a part whose first entry is out of range after `shift`, and P, P and P, -P as a
part's first two entries.  The host twin runs the same jobs on the CPU tier (tests/test_parts_host.py)."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc
import parts_cases as qc
import pass_cases as pc

pytestmark = pytest.mark.gpu

G16_OK, G16_ERR_BAD_ARG = 0, 3
CONFIGS = qc.configs()
CONFIG_IDS = [qc.config_id(*cfg) for cfg in CONFIGS]
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


def call(lab, cfg, jobs, **kw):
    from groth16_amd import binding

    lib, ctxs = lab
    curve, g2, merged, lmax = cfg
    m = pc.model(curve, g2).m
    args = dict(c=pc.C_BITS, groups=pc.GROUPS, G=pc.REDUCE_G, lmax=lmax, rows=pc.ROWS if merged else 1)
    args.update(kw)
    return binding.msm_parts_lab(lib, ctxs[curve], g2, merged, args["c"], args["groups"], args["G"], args["lmax"], args["rows"], jobs, m.words,
                                 (4 if g2 else 2) * m.cp.fq_limbs64)


def alone(lab, cfg, name):
    if (cfg, name) not in RESULTS:
        status, res = call(lab, cfg, [qc.lab_job(qc.job(*cfg, name))])
        assert status == G16_OK, "%s: status %d" % (name, status)
        RESULTS[(cfg, name)] = res[0]
    return RESULTS[(cfg, name)]


CASES = [(cfg, name) for cfg in CONFIGS for name in qc.job_names(cfg[2])]


@pytest.mark.parametrize("cfg,name", CASES, ids=["%s-%s" % (qc.config_id(*cfg), name) for cfg, name in CASES])
def test_parts_job(lab, cfg, name):
    v = qc.job(*cfg, name)
    res = alone(lab, cfg, name)
    if v.S == 0:
        assert res["records"].shape[0] == qc.GUARDS    # nothing launched, nothing written: check() looks at the guards
    qc.check(v, res)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_four_jobs_in_one_launch(lab, cfg):
    views = [qc.job(*cfg, name) for name in qc.BATCH]
    status, res = call(lab, cfg, [qc.lab_job(v) for v in views])
    assert status == G16_OK
    for v, got in zip(views, res):
        qc.check(v, got)
        one = alone(lab, cfg, v.name)
        for key in ("records", "offsets", "task_off", "out"):
            assert (got[key] == one[key]).all(), "%s: %s differs from what the job gave alone" % (v.name, key)
        assert sorted(got["heavy"][1:1 + got["heavy"][0]]) == sorted(one["heavy"][1:1 + one["heavy"][0]])


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[3] == 19], ids=[i for c, i in zip(CONFIGS, CONFIG_IDS) if c[3] == 19])
def test_parts_lab_refusals(lab, cfg):
    """the refusals of the pass lab: whatever would let the kernel read outside what was uploaded; an index out of range after `shift`
    is not refused"""
    curve, g2, merged, lmax = cfg
    base = qc.lab_job(qc.job(*cfg, "first_entries"))
    ok = lambda **kw: call(lab, cfg, [dict(base, **{k: v for k, v in kw.items() if k in base or k in ("n_sorted", "record_cap")})],  # noqa: E731
                           **{k: v for k, v in kw.items() if k not in base and k not in ("n_sorted", "record_cap")})[0]
    counts = base["counts"].copy()
    counts[5] += 1
    assert ok(counts=counts) == G16_ERR_BAD_ARG                                   # sum(counts) != len(sorted)
    assert ok(sorted=base["sorted"][:-1]) == G16_ERR_BAD_ARG
    for bad in (7, 0, 4097, -1):
        assert ok(lmax=bad) == G16_ERR_BAD_ARG, bad
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
    qc.check(qc.job(*cfg, "first_entries"), res[0])
