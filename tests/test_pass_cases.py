"""CPU tier: the generators of the pass lab and the sort lab (tests/pass_cases.py) against the model alone.  Every job asserts, while it
is built, the event it is named after -- a cancellation, a doubling, an identity share, a skipped entry, a segment count -- so building
them all is the test.  Also: the digit-edge scalars hold the digits they are named after, and the two lab structs of the C ABI have the
layout the binding gives them."""
import ctypes as C

import pytest

import pass_cases as pc
import pymodel as pm

CONFIGS = pc.configs()
CP = {"bls12_381": pm.BLS12_381, "bn254": pm.BN254}


@pytest.mark.parametrize("cfg", CONFIGS, ids=[pc.config_id(*cfg) for cfg in CONFIGS])
def test_pass_jobs_hold_their_events(cfg):
    curve, g2, merged, lseg = cfg
    want = {
        "boundaries": {"bucket 0 empty", "bucket M-1 empty", "runs of 1, 2 and 31 empty buckets inside one segment", "an empty run across the group boundary"},
        "last_bucket_only": {"buckets 0..M-2 empty"},
        "segments": {"HEAVY_PARTS segments: not heavy", "HEAVY_PARTS + 1 segments: heavy", "neighbours share the first and the last segment"},
        "collisions": {"[P, -P]", "[P, -P] before the flush inside the loop", "[P, -P, Q]", "[P, P]", "[P, P, -2P]", "the combine cancels", "the combine doubles",
                       "a share of skipped entries only", "skipped first", "skipped last", "skipped between P and -P"},
        "shift_minus_1": {"shift = -1: some entries skipped, some not"},
        "shift_plus_1": {"shift = +1: some entries skipped, some not"},
        "shift_minus_n": {"shift = -n: every entry skipped"},
        "base_count_below": {"base_count below the largest index"},
        "rows": {"every row 0..12; sign bit on row 12 at index base_count - 1"},
        "bit26": {"bit 26 and above set: skipped"},
    }
    names = pc.job_names(merged)
    assert ("rows" in names) == merged and ("bit26" in names) == (not merged) and len(names) == len(pc.JOBS) - 1
    for name in names:
        job = pc.job(*cfg, name)
        assert want.get(name, set()) <= job.seen, (name, want[name] - job.seen)
        assert len(job.counts) == pc.M and sum(job.counts) == len(job.sorted) == job.S and len(job.expected) == job.task_off[pc.M]
        assert all(0 <= v < 1 << 32 for v in job.sorted)
        if merged:
            assert all((v >> 26) & 31 < job.rows for v in job.sorted)     # what the lab would refuse otherwise
    sizes = {name: pc.job(*cfg, name).S for name in names if name.startswith("S")}
    T = pc.TASKS_PER_WG[g2]
    assert sizes == {"S0": 0, "S1": 1, "S_lseg": lseg, "S_lseg_plus_1": lseg + 1, "S_second_workgroup": T * lseg + 1}
    batch = [pc.job(*cfg, name) for name in pc.BATCH]
    assert len({j.S for j in batch}) == 4 and 0 in {j.S for j in batch} and len({(tuple(j.table), j.shift, j.base_count) for j in batch}) >= 3


def test_named_cases_are_the_same_for_every_configuration():
    ref = {name: sorted(pc.job(*CONFIGS[0], name).named) for name in pc.job_names(False)}
    assert sum(len(v) for v in ref.values()) >= 30
    for cfg in CONFIGS:
        for name in pc.job_names(cfg[2]):
            if name in ref:
                assert sorted(pc.job(*cfg, name).named) == ref[name]


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_digit_edge_scalars_hold_their_digits(curve):
    r = CP[curve].r
    for c in list(range(3, 21)):
        W = (r.bit_length() + 1 + c - 1) // c      # at least as many windows as any plan takes for this c
        half = 1 << (c - 1)
        pool = pc.digit_edge_scalars(r, c, W)
        assert len(pool) == len(set(pool)) and all(0 <= s < r for s in pool) and {0, 1, r - 1, (r - 1) // 2, (r + 1) // 2} <= set(pool)
        ds = [pc.digits(s, c, W) for s in pool]
        lows = {w for d in ds for w, x in enumerate(d) if x == -half}
        highs = {w for d in ds for w, x in enumerate(d) if x == half - 1}
        top = max(w for d in ds for w, x in enumerate(d) if x)
        assert set(range(top)) <= lows, (c, sorted(set(range(top)) - lows))      # -2^(c-1): bucket B - 1 with the sign set, every window below the top
        assert set(range(top)) <= highs, (c, sorted(set(range(top)) - highs))
        assert any(all(x == half - 1 for x in d[:top]) for d in ds)               # every digit 2^(c-1) - 1 below the top


def test_digits_refuse_what_does_not_fit():
    with pytest.raises(AssertionError):
        pc.digits(1 << 12, 4, 3)
    assert pc.digits(8, 4, 2) == [-8, 1] and pc.digits(7, 4, 2) == [7, 0] and pc.digits(0xF8, 4, 3) == [-8, 0, 1]


def test_lab_structs_have_the_binding_layout():
    from groth16_amd import binding

    lb = binding.lib()
    assert lb.c.g16_struct_size(8) == C.sizeof(binding.PassLabJobC) == 104
    assert lb.c.g16_struct_size(9) == C.sizeof(binding.SortLabInfoC) == 80
    assert binding.PassLabJobC.records.offset == 56 and binding.PassLabJobC.out_affine.offset == 96 and binding.SortLabInfoC.K.offset == 32
    assert lb.c.g16_struct_size(10) == 0
