"""GPU tier: the reductions of SEVERAL MSMs in one launch per kernel -- msm_reduce_batch and msm_heavy_reduce_batch, which every proof
uses for its G1 MSMs -- through g16_dev_msm_reduce_batch_lab, on jobs that can be told apart (tests/reduce_cases.py: BATCHES,
batch_conditions; test_reduce_cases.py asserts the conditions without a GPU).  heavy_reduce_kernel, bucket_combine_kernel,
bucket_reduce_kernel and window_reduce_kernel pick their MSM with blockIdx.y / .z out of per-MSM pointers (partial sums, slot offsets,
heavy list, chunk sums, group sums); whole proofs cannot tell a wrong index from a right one, because l, a and b_g1 share one sort and
h's heavy list is empty on random data.

G1 only (the prover batches no G2 reductions), both curves, per-window and merged fold, 8 / 16 / 32 buckets per reduction lane.  One
lab call per (configuration, batch, mode); the modes are the two ways prove_partial launches the stages:
  together   msm_reduce_batch(all jobs, heavy_done = false): the last batch of a proof with h inside
  early      a subset's first stage in one launch (msm_heavy_reduce_batch), every other job's alone (msm_heavy_reduce), then
             msm_reduce_batch(all jobs, heavy_done = true): the single-GPU proof, subset {0, 1, 2} = l, a, b_g1
For every job: every bucket's first slot decodes to the model's bucket sum, the folded point is the model's, and both equal BIT FOR
BIT what the job gives alone through g16_dev_msm_reduce_lab -- every kernel's gridDim.x is the same for one job or four and the
additions inside a job do not depend on the batch, so the lazy limbs must not either.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc
import reduce_cases as rc
from helpers import arr_to_g1

pytestmark = pytest.mark.gpu

CONFIGS = rc.batch_configs()
CONFIG_IDS = [rc.config_id(*cfg) for cfg in CONFIGS]
RUNS = [(batch, mode) for batch in rc.BATCHES for mode in rc.batch_modes(batch)]
RUN_IDS = ["%s-%s" % ("+".join(b), "together" if m is None else "early" + "".join(map(str, m))) for b, m in RUNS]
ALONE, BATCHED = {}, {}   # one lab call each, shared by the tests that read it


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


def job_arrays(sc):
    return np.array(sc.nparts, dtype=np.uint32), np.array(sc.records, dtype=np.uint32).reshape(len(sc.records), sc.m.words)


def alone(lab, cfg, name):
    """the job through the existing lab: msm_reduce, the batch of one"""
    if (cfg, name) not in ALONE:
        from groth16_amd import binding

        lib, ctxs = lab
        curve, g2, merged, chunk = cfg
        sc = rc.scenario(*cfg, name)
        nparts, records = job_arrays(sc)
        ALONE[(cfg, name)] = binding.msm_reduce_lab(lib, ctxs[curve], False, merged, rc.C_BITS, rc.GROUPS, chunk, nparts, records,
                                                    2 * sc.m.cp.fq_limbs64)
    return ALONE[(cfg, name)]


def batched(lab, cfg, batch, mode):
    if (cfg, batch, mode) not in BATCHED:
        from groth16_amd import binding

        lib, ctxs = lab
        curve, g2, merged, chunk = cfg
        scs = [rc.scenario(*cfg, name) for name in batch]
        # (a scenario that is in the batch twice goes in as two separate copies of its arrays)
        status, outs = binding.msm_reduce_batch_lab(lib, ctxs[curve], merged, rc.C_BITS, rc.GROUPS, chunk, [job_arrays(sc) for sc in scs],
                                                    early=mode, affine_words=2 * scs[0].m.cp.fq_limbs64)
        lib.check(status)
        BATCHED[(cfg, batch, mode)] = outs
    return BATCHED[(cfg, batch, mode)]


def where(batch, y, mode):
    return "job %d (%s) of the batch %s, mode %s" % (y, batch[y], "+".join(batch), "together" if mode is None else "early, subset %s" % (mode,))


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_every_job_of_the_batch(lab, cfg, run):
    batch, mode = run
    outs = batched(lab, cfg, batch, mode)
    assert len(outs) == len(batch)
    for y, name in enumerate(batch):
        sc = rc.scenario(*cfg, name)
        first, out = outs[y]
        total = arr_to_g1(out, sc.m.cp)[0]
        for b in range(rc.GROUPS * rc.B):
            got, want = sc.m.decode(first[b]), sc.sums[b]
            assert got == want, "%s: bucket %d (group %d, bucket %d; %d partial sums; %s): first slot holds %s, the bucket's sum is %s" % (
                where(batch, y, mode), b, b // rc.B, b % rc.B, sc.nparts[b], sc.named.get(b, "unnamed"),
                "the identity" if got is None else got, "the identity" if want is None else want)
        assert total == sc.total, "%s: folded sum %s, model %s" % (where(batch, y, mode), total, sc.total)
        first_1, out_1 = alone(lab, cfg, name)
        same = (first == first_1).all(axis=1)
        assert same.all(), "%s: the first slots of buckets %s are the right points but not the limbs the job gives alone" % (
            where(batch, y, mode), np.nonzero(~same)[0].tolist())
        assert (out == out_1).all(), where(batch, y, mode)


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[-1]], ids=[CONFIG_IDS[0], CONFIG_IDS[-1]])
def test_batch_lab_refusals(lab, cfg):
    from groth16_amd import binding

    lib, ctxs = lab
    curve, g2, merged, chunk = cfg
    sc = rc.scenario(*cfg, "single")
    job = job_arrays(sc)
    aw = 2 * sc.m.cp.fq_limbs64

    def call(jobs, early=None, G=chunk):
        return binding.msm_reduce_batch_lab(lib, ctxs[curve], merged, rc.C_BITS, rc.GROUPS, G, jobs, early=early, affine_words=aw)[0]

    BAD_ARG, BAD_LENGTH = 3, 2
    assert call([]) == BAD_ARG                                  # no job
    assert call([job] * 5) == BAD_ARG                            # more than four
    assert call([job] * 5, early=(0,)) == BAD_ARG
    assert call([job, job], early=()) == BAD_ARG                 # early mode, empty subset
    assert call([job, job], early=(2,)) == BAD_ARG               # a job that is not there
    assert call([job], G=4) == BAD_ARG                           # (the plan's own refusals, as in the lab of one)
    assert call([job, (job[0], job[1][:0])]) == BAD_LENGTH       # records that are not the sum of nparts
    assert call([job, job], early=(1,)) == 0 and call([job] * 4) == 0
