"""CPU tier: the generators of the group-arithmetic labs against the model alone.  Every case of tests/fp30_cases.py::parked_cases and
every scenario of tests/reduce_cases.py that is named after a doubling or a cancellation asserts, while it is built, that the model
meets one there; building them all is the test.  Also: a record written by the generator decodes to its point, for every
representative the producers promise."""
import random

import pytest

import fp30_cases as fc
import reduce_cases as rc

CONFIGS = rc.configs()


@pytest.mark.parametrize("cfg", CONFIGS, ids=[rc.config_id(*cfg) for cfg in CONFIGS])
def test_reduction_scenarios_hold_their_collisions(cfg):
    curve, g2, merged, chunk = cfg
    want = {"combine": {"bucket_combine_kernel: [O, P, -P]", "bucket_combine_kernel: [P, P] with two scales", "heavy_reduce_kernel: the tree doubles",
                        "heavy_reduce_kernel: the tree cancels", "heavy_reduce_kernel: a task's run is [P, -P]",
                        "window_reduce_kernel: a group whose chunks are all empty"},
            "chains": {"bucket_reduce_kernel: run doubles (equal sums in adjacent buckets)", "bucket_reduce_kernel: tot += run adds a record to itself",
                       "bucket_reduce_kernel: run cancels and restarts", "bucket_reduce_kernel: tot cancels and restarts"}}
    if chunk < rc.B:
        want["chains"] |= {"window_reduce_kernel: chunks with equal sums", "window_reduce_kernel: chunks with opposite sums"}
    for name in rc.SCENARIOS:
        sc = rc.scenario(*cfg, name)
        assert want[name] <= sc.seen, want[name] - sc.seen
        assert len(sc.nparts) == rc.GROUPS * rc.B and sum(sc.nparts) == len(sc.records)
        assert all(len(r) == sc.m.words for r in sc.records)
        assert len(sc.records) < 400   # a few hundred records per call
    sc = rc.scenario(*cfg, "combine")
    counts = {sc.nparts[b] for b in sc.named}
    assert {rc.HEAVY_PARTS, rc.HEAVY_PARTS + 1} <= counts and max(counts) > rc.HEAVY_TASKS[g2]
    by_name = {v: b for b, v in sc.named.items()}
    assert sc.sums[by_name["bucket_combine_kernel [O, P, -P]"]] is None and sc.nparts[by_name["bucket_combine_kernel [O, P, -P]"]] == 3


BATCH_CONFIGS = rc.batch_configs()


@pytest.mark.parametrize("cfg", BATCH_CONFIGS, ids=[rc.config_id(*cfg) for cfg in BATCH_CONFIGS])
def test_batch_jobs_can_be_told_apart(cfg):
    """The jobs of every batch of the batch lab differ where a reduction kernel that read another job's heavy list, slot offsets or
    buffers would go wrong: rc.batch_conditions asserts it, with the model alone, for every job behind index 0."""
    curve, _, merged, chunk = cfg
    M = rc.GROUPS * rc.B
    comb, comp = rc.scenario(*cfg, "combine"), rc.scenario(*cfg, "complement")
    Hc, Hp = set(rc.heavy_buckets(comb)), set(rc.heavy_buckets(comp))
    assert {0, M - 1} <= Hp and not Hc & Hp and len(Hc) >= 2
    assert any(comp.nparts[b] == 0 and comp.nparts[b + 1] == 1 and comp.sums[b + 1] is not None for b in Hc)
    assert any(2 <= comp.nparts[b] <= rc.HEAVY_PARTS for b in Hc)
    assert sum(comp.nparts) != sum(comb.nparts)
    assert sum(rc.scenario(*cfg, "empty").nparts) == 0 and sorted(rc.scenario(*cfg, "single").nparts)[-2:] == [0, 1]
    for name in rc.BATCH_SCENARIOS:
        sc = rc.scenario(*cfg, name)
        assert len(sc.nparts) == M and sum(sc.nparts) == len(sc.records) < 400
    assert [b for b in rc.BATCHES if len(b) == 4][0][::-1] == [b for b in rc.BATCHES if len(b) == 4][1]
    assert any(b[0] == "complement" and b[3:] == ("combine",) for b in rc.BATCHES) and ("complement", "combine") in rc.BATCHES
    assert ("combine", "combine") in rc.BATCHES and ("single",) in rc.BATCHES and any(len(b) == 3 for b in rc.BATCHES)
    assert all(len(b) <= 4 for b in rc.BATCHES)
    for batch in rc.BATCHES:
        held = rc.batch_conditions(curve, merged, chunk, batch)
        assert sorted(held) == list(range(1, len(batch)))
        for y, name in enumerate(batch):
            if y and name in ("combine", "complement") and name != batch[0]:
                assert {"heavy", "offsets"} <= held[y], (batch, y, held[y])
        if batch[:1] == ("combine",) and "complement" in batch:
            assert {"overwrite, adjacent", "twice"} <= held[batch.index("complement")]
    assert rc.EARLY_SUBSETS[4] == ((0, 1, 2), (0,), (1, 2)) and (1, 2) in rc.EARLY_SUBSETS[3]


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_records_decode_to_their_points(curve, g2):
    m = rc.model(curve, g2)
    rng = random.Random(7)
    p = m.f.p
    assert m.decode(m.record(None, rng)) is None
    for kx in range(7):
        for ky in range(4):
            P = m.pts[(5 * kx + ky) % len(m.pts)]
            rec = m.record(P, rng, kx, ky)
            assert len(rec) == m.words and m.decode(rec) == P
            NL, C = m.f.NL, m.C
            vals = [m.f.value(rec[i * NL:(i + 1) * NL]) for i in range(4 * C)]
            assert all(kx * p <= v < (kx + 1) * p for v in vals[:C]) and all(ky * p <= v < (ky + 1) * p for v in vals[C:2 * C])
            assert all(5 * v < 9 * p for v in vals[2 * C:])   # zz, zzz < 1.8 p


@pytest.mark.parametrize("f", [f for f in fc.fields() if f.which == "fq"], ids=lambda f: f.name)
@pytest.mark.parametrize("form", ["parked_chain_g1", "parked_chain_g2_pair"])
def test_parked_cases_hold_their_collisions(f, form):
    cases = fc.lab_cases(f, form)   # the assertions are in the generator
    assert len(cases) >= 65
    fid, nin, nout = fc.LAB[form]
    assert all(len(c.slots) == nin and all(len(s) == f.NL for s in c.slots) for c in cases)
