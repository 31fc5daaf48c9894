"""The model of the bucket-part walk's layout, jobs for the parts lab (g16_dev_msm_parts_lab, g16_host_msm_parts_lab) and the check of
a lab result against the model (TEST INFRASTRUCTURE).

The part walk (groth16_amd/csrc/part_walk.hpp) cuts a bucket of n > 0 entries into np = ceil(n / Lmax) parts; part p covers the entries
[off + p n // np, off + (p + 1) n // np) of the sorted list, slot task_off[b] + p holds its signed sum, and a lane walks exactly one part.
Rules of the model:
  task_off          exclusive prefix of ceil(n_b / Lmax)
  heavy (a set)     the buckets with more than HEAVY_PARTS parts
  record of slot    the signed sum of exactly the part's entries, skipped entries left out (pass_cases.Job.decode)
  fold              as in pass_cases
The jobs are those of tests/pass_cases.py -- the entries, tables, shifts and base_counts; only the cut into tasks differs -- plus the
ones below, which place what the part walk can get wrong: bucket sizes around the part length, a bucket on the heavy list, a task list
whose first wave mixes trip counts, one whose tasks all have one length, a part whose first entry is skipped, and a doubling and a
cancellation on a part's first two entries.  Every event a job is named after is asserted with the model alone while it is built."""
import functools
import random
import struct

import numpy as np

import fp30_cases as fc
import pass_cases as pc

LMAXS = pc.LSEGS
M, HEAVY_PARTS, GUARDS, FILL_WORD = pc.M, pc.HEAVY_PARTS, pc.GUARDS, pc.FILL_WORD


def layout(counts, lmax):
    """(offsets, nparts, task_off, parts) of a bucket histogram; parts[slot] = (bucket, part, start, length)"""
    offsets, nparts, task_off, parts = [0], [], [0], []
    for b, n in enumerate(counts):
        np_ = -(-n // lmax)
        for p in range(np_):
            lo, hi = offsets[-1] + p * n // np_, offsets[-1] + (p + 1) * n // np_
            parts.append((b, p, lo, hi - lo))
        offsets.append(offsets[-1] + n)
        nparts.append(np_)
        task_off.append(task_off[-1] + np_)
    return offsets, nparts, task_off, parts


def slot_bound(S, n_buckets, lmax):
    """the host's upper bound on the slots: entries / Lmax + buckets"""
    return S // lmax + n_buckets


class Parts:
    """a pass_cases.Job seen through the part layout with longest part lmax"""

    def __init__(self, job, lmax):
        self.job, self.lmax, self.pm, self.name, self.named = job, lmax, job.pm, job.name, job.named
        self.merged, self.shift, self.base_count = job.merged, job.shift, job.base_count
        self.counts = [len(q) for q in job.buckets]
        self.sorted = [v for q in job.buckets for v in q]
        self.S = len(self.sorted)
        self.offsets, self.nparts, self.task_off, self.parts = layout(self.counts, lmax)
        self.heavy = {b for b, n in enumerate(self.nparts) if n > HEAVY_PARTS}
        r = self.pm.r
        self.shares, self.tags, self.expected = [], [], []
        self.sums = [0] * M
        for b, p, lo, n in self.parts:
            ks = [job.decode(v) for v in self.sorted[lo:lo + n]]
            acc, tags = 0, []
            for k in ks:
                tags.append(pc.tag_add(acc, k or 0, r))
                acc += k or 0
            self.shares.append(ks)
            self.tags.append(tags)
            self.expected.append(acc)
            self.sums[b] += acc
        assert len(self.expected) == self.task_off[M] <= slot_bound(self.S, M, lmax)
        if self.merged:
            self.total = sum((k + 1) * s for k, s in enumerate(self.sums))
        else:
            self.total = sum((sum((b + 1) * self.sums[w * pc.B + b] for b in range(pc.B))) << (pc.C_BITS * w) for w in range(pc.GROUPS))

    def slots(self, b):
        return range(self.task_off[b], self.task_off[b + 1])

    def lengths(self):
        """the task list's lengths in launch order: longest first"""
        return sorted((n for _, _, _, n in self.parts), reverse=True)

    def table_points(self):
        return self.job.table_points()


# ---- the jobs of this module -----------------------------------------------------------------------------------------------------------
def _sizes(job, rng, L):
    F = lambda n: job.fill(rng, n)   # noqa: E731
    job.skip(1)                                                   # bucket 0: size 0
    names = {1: "a bucket of 1 entry", L: "a bucket of Lmax entries", L + 1: "a bucket of Lmax + 1 entries", 2 * L: "a bucket of 2 Lmax entries",
             2 * L + 1: "a bucket of 2 Lmax + 1 entries"}
    at = {}
    for n, name in names.items():
        at[n] = job.bucket(F(n), name)
        job.skip(1)                                               # size 0 between them
    job.bucket(F(3))
    return lambda v: _sizes_check(v, at, L)


def _sizes_check(v, at, L):
    want = {1: [1], L: [L], L + 1: [(L + 1) // 2, L + 1 - (L + 1) // 2], 2 * L: [L, L], 2 * L + 1: None}
    assert v.counts[0] == 0 and v.nparts[0] == 0
    for n, b in at.items():
        got = [ln for bb, _, _, ln in v.parts if bb == b]
        assert sum(got) == n and max(got) <= L and max(got) - min(got) <= 1
        if want[n]:
            assert got == want[n], (n, got)
        assert v.counts[b + 1] == 0
    assert len([1 for bb, _, _, _ in v.parts if bb == at[2 * L + 1]]) == 3 and v.nparts[at[L + 1]] == 2
    return {"sizes 0, 1, Lmax, Lmax + 1, 2 Lmax, 2 Lmax + 1"}


def _heavy(job, rng, L):
    job.skip(2)
    n1 = job.bucket(job.fill(rng, HEAVY_PARTS * L), "a bucket of exactly HEAVY_PARTS Lmax entries")
    h = job.bucket(job.fill(rng, HEAVY_PARTS * L + 1), "a bucket of more than HEAVY_PARTS Lmax entries")
    job.bucket(job.fill(rng, 2))

    def check(v):
        assert v.nparts[n1] == HEAVY_PARTS and v.nparts[h] == HEAVY_PARTS + 1 and v.heavy == {h}
        return {"HEAVY_PARTS parts: not heavy", "HEAVY_PARTS + 1 parts: heavy"}
    return check


def _mixed_wave(job, rng, L):
    """more than 64 tasks of several lengths: the first wave of the launch (64 tasks, or 32 lane pairs) mixes trip counts"""
    for _ in range(30):
        job.bucket(job.fill(rng, 2 * L + 3))
    for _ in range(10):
        job.bucket(job.fill(rng, L))
    job.bucket(job.fill(rng, 1))

    def check(v):
        ls = v.lengths()
        T = pc.TASKS_PER_WG[v.pm.g2]
        assert len(ls) >= 65 and len(set(ls)) >= 3
        waves = [ls[i:i + T] for i in range(0, len(ls), T)]
        assert any(len(set(w)) >= 2 for w in waves) and len(waves) >= 2
        assert len(ls) % T != 0                                   # the last wave is partly idle
        return {"a wave of two trip counts"}
    return check


def _one_length(job, rng, L):
    for k in range(24):
        job.bucket(job.fill(rng, L if k % 3 else 2 * L))
        job.skip(k % 2)

    def check(v):
        assert set(v.lengths()) == {L} and len(v.parts) == 32
        return {"every task of one length"}
    return check


def _first_entries(job, rng, L):
    """shift = -1 as in pass_cases' collisions: the raw point index 0 leaves the range"""
    assert job.shift == -1
    P, P2, nP2, Q = job.word(pc.I_P), job.word(pc.I_P2), job.word(pc.I_P2, True), job.word(pc.I_Q)
    OUT = 0 | (1 << 31)
    F = lambda n: job.fill(rng, n)   # noqa: E731
    job.skip(3)
    a = job.bucket([OUT, P, Q], "a part whose first entry is out of range")
    b = job.bucket([OUT, OUT, P, Q], "a part whose first two entries are out of range")
    c = job.bucket([P, P2, Q], "a part that starts P, P")
    d = job.bucket([P, nP2, Q], "a part that starts P, -P")
    e = job.bucket([P, P2], "a part that is P, P")
    f = job.bucket([P, nP2], "a part that is P, -P")
    g = job.bucket([OUT], "a part that is one entry out of range")
    # a bucket of two parts whose SECOND part starts with the entry out of range, then P, P
    first = F(L)
    second = [OUT, P, P2] + F(L - 3)
    h = job.bucket(first + second, "a second part that starts out of range, then P, P")

    def check(v):
        T = lambda bb: [v.tags[s] for s in v.slots(bb)]   # noqa: E731
        kP, kQ = pc.K_P, pc.K_Q
        assert T(a) == [["skip", "copy", "hot"]] and v.sums[a] == kP + kQ
        assert T(b) == [["skip", "skip", "copy", "hot"]] and v.sums[b] == kP + kQ
        assert T(c) == [["copy", "dbl", "hot"]] and v.sums[c] == 2 * kP + kQ
        assert T(d) == [["copy", "cancel", "copy"]] and v.sums[d] == kQ
        assert T(e) == [["copy", "dbl"]] and T(f) == [["copy", "cancel"]] and v.sums[f] == 0
        assert T(g) == [["skip"]] and v.expected[v.task_off[g]] == 0
        assert v.nparts[h] == 2 and T(h)[1][:3] == ["skip", "copy", "dbl"] and [ln for bb, _, _, ln in v.parts if bb == h] == [L, L]
        return {"first entry out of range", "P, P first", "P, -P first", "an identity record that the walk must write"}
    return check


# name -> (generator, pass_cases.Job keywords)
NEW_JOBS = {
    "sizes": (_sizes, {}),
    "heavy": (_heavy, {}),
    "mixed_wave": (_mixed_wave, {}),
    "one_length": (_one_length, {}),
    "first_entries": (_first_entries, {"shift": -1}),
}
BATCH = ("sizes", "S0", "first_entries", "base_count_below")


def job_names(merged):
    return list(NEW_JOBS) + pc.job_names(merged)


@functools.lru_cache(maxsize=None)
def job(curve, g2, merged, lmax, name):
    """the Parts view of a job; `seen` holds the events the generator asserted"""
    if name in NEW_JOBS:
        make, kw = NEW_JOBS[name]
        j = pc.Job(pc.model(curve, g2), merged, lmax, name, **kw)
        check = make(j, random.Random("parts/%s/%d/%d/%d/%s" % (curve, g2, merged, lmax, name)), lmax)
        v = Parts(j, lmax)
        v.seen = check(v)
    else:
        v = Parts(pc.job(curve, g2, merged, lmax, name), lmax)
        v.seen = set()
    assert v.S <= 1 << 16
    return v


configs, config_id = pc.configs, pc.config_id


def lab_job(v):
    cp = v.pm.m.cp
    from helpers import g1_to_arr, g2_to_arr

    table = (g2_to_arr if v.pm.g2 else g1_to_arr)(v.table_points(), cp)
    return {"table": table, "base_count": v.base_count, "shift": v.shift, "counts": np.array(v.counts, dtype=np.uint32),
            "sorted": np.array(v.sorted, dtype=np.uint32)}


def show(P):
    return "the identity" if P is None else str(P)


def check(v, res, guards=GUARDS):
    """a lab result against the model: the layout, every slot written, every record (named buckets first), the guards, the fold"""
    from helpers import arr_to_g1, arr_to_g2

    pm, m = v.pm, v.pm.m
    assert [int(x) for x in res["offsets"]] == v.offsets, "offsets are not the exclusive prefix of the counts"
    assert [int(x) for x in res["task_off"]] == v.task_off, "task_off is not the exclusive prefix of ceil(count / Lmax)"
    nh = int(res["heavy"][0])
    assert nh == len(v.heavy) and {int(b) for b in res["heavy"][1:1 + nh]} == v.heavy, "heavy list %s, buckets with more than %d parts: %s" % (
        list(res["heavy"][:1 + nh]), HEAVY_PARTS, sorted(v.heavy))
    records = res["records"]
    n = v.task_off[M]
    assert records.shape == (n + guards, m.words)
    names = {b: name for name, b in v.named.items()}
    zz = slice(2 * m.C * m.f.NL, 3 * m.C * m.f.NL)
    bad = []
    for slot in sorted(range(n), key=lambda s: (v.parts[s][0] not in names, s)):
        b, p, lo, ln = v.parts[slot]
        what = "%s: bucket %d, part %d (slot %d, entries [%d, %d) as multiples of G: %s)" % (names.get(b, "an unnamed bucket"), b, p, slot, lo, lo + ln, v.shares[slot])
        if (records[slot][zz] == FILL_WORD).all():
            bad.append(what + ": never written, the slot still holds the fill")
            continue
        got, want = m.decode(records[slot]), pm.point(v.expected[slot])
        if got != want:
            bad.append(what + ": the record holds %s, the part's sum is %s" % (show(got), show(want)))
    assert not bad, "%s, %d of %d records wrong:\n%s" % (v.name, len(bad), n, "\n".join(bad[:6]))
    if guards:
        assert (records[n:] == FILL_WORD).all(), "%s: a guard record behind slot %d changed" % (v.name, n)
    got = (arr_to_g2 if pm.g2 else arr_to_g1)(res["out"], m.cp)[0]
    assert got == pm.point(v.total), "%s: folded sum %s, model %s" % (v.name, show(got), show(pm.point(v.total)))


# ---- the job file of tests/parts_walk_replay.cpp -----------------------------------------------------------------------------------------
def dump_jobs(path, items):
    """items: (curve id, merged, lmax, rows, lab job dict, host-twin result) -- one record each, little-endian: 12 uint32 (curve, merged,
    c, groups, lmax, rows, base_count, n_sorted, M, affine words, record words, n_records), shift as int64, then the table (uint64),
    counts, sorted, and this build's task_off, records (uint32) and folded sum (uint64)"""
    with open(path, "wb") as fh:
        for curve_id, merged, lmax, rows, lj, res in items:
            table = np.ascontiguousarray(lj["table"], dtype=np.uint64)
            aff = table.shape[1] if table.ndim == 2 and table.shape[0] else len(res["out"])
            rec = res["records"]
            fh.write(struct.pack("<12Iq", curve_id, int(merged), pc.C_BITS, pc.GROUPS, lmax, rows, int(lj["base_count"]), len(lj["sorted"]), M, aff,
                                 rec.shape[1], rec.shape[0], int(lj["shift"])))
            for a, dt in ((table, np.uint64), (lj["counts"], np.uint32), (lj["sorted"], np.uint32), (res["task_off"], np.uint32), (rec, np.uint32),
                          (res["out"], np.uint64)):
                fh.write(np.ascontiguousarray(a, dtype=dt).tobytes())


CURVE_ID = fc.CURVE_ID
