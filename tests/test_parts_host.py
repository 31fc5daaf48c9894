"""CPU tier: the bucket-part walk off the GPU.  The layout model of tests/parts_cases.py holds its properties on random histograms; the
jobs of the parts lab hold the events they are named after; and the host twin (g16_host_msm_parts_lab: the layout rule and the per-task
walk of groth16_amd/csrc/part_walk.hpp, the code the bucket pass runs per lane, compiled for the host) gives on every G1 job what the
model gives -- task_off, the heavy list, every record as the signed sum of exactly its part, the fold.  The same jobs, with the twin's
outputs, are written as the job file of tests/parts_walk_replay.cpp, the stand-alone program for a sanitizer build."""
import random
import struct

import numpy as np
import pytest

import parts_cases as qc
import pass_cases as pc

G16_OK, G16_ERR_BAD_ARG, G16_ERR_BAD_LENGTH = 0, 3, 2
CONFIGS = qc.configs()
G1_CONFIGS = [cfg for cfg in CONFIGS if not cfg[1]]


@pytest.mark.parametrize("lmax", [8, 19, 48, 64, 96, 128, 4096])
def test_layout_model_tiles_every_bucket(lmax):
    rng = random.Random("layout/%d" % lmax)
    for trial in range(40):
        nb = rng.randrange(1, 80)
        top = rng.choice((3, lmax, 3 * lmax, 40 * lmax))
        counts = [rng.choice((0, 0, 1, lmax - 1, lmax, lmax + 1, 2 * lmax, 2 * lmax + 1, rng.randrange(top + 1))) for _ in range(nb)]
        offsets, nparts, task_off, parts = qc.layout(counts, lmax)
        S = sum(counts)
        assert offsets[-1] == S and len(parts) == task_off[-1] <= qc.slot_bound(S, nb, lmax)
        at = 0
        for b, n in enumerate(counts):
            mine = parts[task_off[b]:task_off[b + 1]]
            assert len(mine) == nparts[b] == -(-n // lmax)
            assert [p for _, p, _, _ in mine] == list(range(len(mine))) and all(bb == b for bb, _, _, _ in mine)
            for _, _, lo, ln in mine:                      # the parts tile the bucket exactly, in order
                assert lo == at and 1 <= ln <= lmax
                at += ln
            assert at == offsets[b + 1]
            if mine:
                lens = [ln for _, _, _, ln in mine]
                assert max(lens) - min(lens) <= 1 and sum(ln == n // len(mine) + 1 for ln in lens) == n % len(mine)


@pytest.mark.parametrize("cfg", CONFIGS, ids=[qc.config_id(*cfg) for cfg in CONFIGS])
def test_parts_jobs_hold_their_events(cfg):
    want = {"sizes": {"sizes 0, 1, Lmax, Lmax + 1, 2 Lmax, 2 Lmax + 1"}, "heavy": {"HEAVY_PARTS parts: not heavy", "HEAVY_PARTS + 1 parts: heavy"},
            "mixed_wave": {"a wave of two trip counts"}, "one_length": {"every task of one length"},
            "first_entries": {"first entry out of range", "P, P first", "P, -P first", "an identity record that the walk must write"}}
    for name in qc.job_names(cfg[2]):
        v = qc.job(*cfg, name)
        assert want.get(name, set()) <= v.seen, name
        assert sum(v.counts) == v.S == len(v.sorted) and len(v.expected) == v.task_off[qc.M]
        assert sorted(s for _, _, s, _ in v.parts) == [s for _, _, s, _ in v.parts]
    assert set(qc.BATCH) <= set(qc.job_names(cfg[2])) and len({qc.job(*cfg, n).S for n in qc.BATCH}) == 4


@pytest.fixture(scope="module")
def lib():
    import groth16_amd

    return groth16_amd.lib()


def host(lib, cfg, lj, **kw):
    from groth16_amd import binding

    curve, g2, merged, lmax = cfg
    m = pc.model(curve, False).m
    args = dict(c=pc.C_BITS, groups=pc.GROUPS, lmax=lmax, rows=pc.ROWS if merged else 1)
    args.update(kw)
    return binding.host_msm_parts_lab(lib, qc.CURVE_ID[curve], merged, args["c"], args["groups"], args["lmax"], args["rows"], lj, m.words,
                                      2 * m.cp.fq_limbs64)


HOST_CASES = [(cfg, name) for cfg in G1_CONFIGS for name in qc.job_names(cfg[2])]


@pytest.mark.parametrize("cfg,name", HOST_CASES, ids=["%s-%s" % (qc.config_id(*cfg), name) for cfg, name in HOST_CASES])
def test_host_twin_job(lib, cfg, name):
    v = qc.job(*cfg, name)
    status, res = host(lib, cfg, qc.lab_job(v))
    assert status == G16_OK
    qc.check(v, res, guards=0)


@pytest.mark.parametrize("cfg", [c for c in G1_CONFIGS if c[3] == 19], ids=[qc.config_id(*c) for c in G1_CONFIGS if c[3] == 19])
def test_host_twin_refusals(lib, cfg):
    curve, g2, merged, lmax = cfg
    base = qc.lab_job(qc.job(*cfg, "first_entries"))
    counts = base["counts"].copy()
    counts[5] += 1
    assert host(lib, cfg, dict(base, counts=counts))[0] == G16_ERR_BAD_ARG
    assert host(lib, cfg, dict(base, sorted=base["sorted"][:-1]))[0] == G16_ERR_BAD_ARG
    for bad in (7, 0, 4097, -1):
        assert host(lib, cfg, base, lmax=bad)[0] == G16_ERR_BAD_ARG, bad
    if merged:
        srt = base["sorted"].copy()
        srt[3] |= pc.ROWS << 26
        assert host(lib, cfg, dict(base, sorted=srt))[0] == G16_ERR_BAD_ARG
        assert host(lib, cfg, base, rows=33)[0] == G16_ERR_BAD_ARG
    else:
        assert host(lib, cfg, base, rows=2)[0] == G16_ERR_BAD_ARG
    assert host(lib, cfg, dict(base, record_cap=len(base["sorted"]) // lmax + qc.M - 1))[0] == G16_ERR_BAD_LENGTH
    assert host(lib, (curve, g2, merged, lmax), base)[0] == G16_OK


def test_layout_launcher_refuses_a_short_lmax(lib):
    """msm_parts_layout (msm_sort.hip, an object of the product library) turns down lmax < 8 with G16_ERR_INTERNAL before it touches the device"""
    import ctypes

    fn = ctypes.CDLL(lib.path)["_ZN3g1616msm_parts_layoutEPKjjjPjS2_S2_S2_PNS_8PartTaskES2_P12ihipStream_t"]
    scratch = (ctypes.c_uint32 * 4)()
    assert fn(None, ctypes.c_uint32(qc.M), ctypes.c_uint32(7), None, None, None, None, None, scratch, None) == 7   # G16_ERR_INTERNAL


def test_job_dump_for_the_replay_program(lib, tmp_path):
    """the file tests/parts_walk_replay.cpp reads: one record per (G1 configuration, job), the job and this build's outputs"""
    items = []
    for cfg in G1_CONFIGS:
        for name in qc.job_names(cfg[2]):
            lj = qc.lab_job(qc.job(*cfg, name))
            status, res = host(lib, cfg, lj)
            assert status == G16_OK
            items.append((qc.CURVE_ID[cfg[0]], cfg[2], cfg[3], pc.ROWS if cfg[2] else 1, lj, res))
    path = tmp_path / "parts_lab.bin"
    qc.dump_jobs(str(path), items)
    raw = path.read_bytes()
    hdr = struct.unpack_from("<12Iq", raw, 0)
    lj, res = items[0][4], items[0][5]
    assert hdr[:6] == (items[0][0], int(items[0][1]), pc.C_BITS, pc.GROUPS, items[0][2], items[0][3])
    assert hdr[7] == len(lj["sorted"]) and hdr[8] == qc.M and hdr[11] == res["records"].shape[0] and hdr[12] == lj["shift"]
    want = sum(56 + 8 * np.asarray(i[4]["table"]).size + 4 * (qc.M + len(i[4]["sorted"]) + qc.M + 1 + i[5]["records"].size) + 8 * len(i[5]["out"])
               for i in items)
    assert len(raw) == want and len(items) == len(HOST_CASES)
