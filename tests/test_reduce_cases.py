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
