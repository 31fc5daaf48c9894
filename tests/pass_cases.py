"""Crafted sorted lists for the pass lab (g16_dev_msm_pass_lab), scalar sets for the sort lab (g16_dev_msm_sort_lab) and the models of
what the bucket pass and the sort make of them (TEST INFRASTRUCTURE).

The pass lab runs bucket_accumulate30_kernel -- the binary search for a segment's first bucket, the flush at a bucket's end, the skip
over empty buckets, the slot index, decode with shift / base_count / the window row, the batch dispatch -- on a sorted list and a bucket
histogram the caller made, so a test can place what whole MSMs never do: the ORDER of entries inside a bucket (LDS atomics decide it in
a real sort), a bucket's position against the segment grid, runs of empty buckets, entries that must be skipped.  The partial-sum slots
are pre-filled with the byte 0xA5, so a slot the walk never wrote shows.

The model works on scalars.  Every table point is a known multiple k G of the group's generator (the identity base (0, 0) is k = 0), so
the signed sum of a share is an integer, and a doubling or a cancellation is an equality of integers mod r (G has prime order r, so
equal points <=> equal scalars).  The expected POINT of a record is pymodel's k G; records are decoded with reduce_cases.Model.decode
and compared as affine points.  Rules:
  record of (bucket b, segment t)   the signed sum of the entries of b that lie in [t lseg, (t + 1) lseg), skipped entries left out
  task_off                          exclusive prefix of the number of segments each non-empty bucket touches
  heavy (a set)                     the buckets that touch more than HEAVY_PARTS segments
  fold                              sum_w 2^(c w) sum_b (b + 1) S_(w,b)  (per-window)  or  sum_k (k + 1) S_k  (merged)
An entry is skipped when its index leaves [0, base_count) after `shift`, or when the base it addresses is the identity.

Every job is named, and every named event in it (cancellation, doubling, identity share, skipped entry, segment count) is asserted by the
generator with the model alone; tests/test_pass_cases.py runs that without a GPU."""
import functools
import os
import random
import re

import fp30_cases as fc
import reduce_cases as rc

C_BITS, GROUPS, B = rc.C_BITS, rc.GROUPS, rc.B
M = GROUPS * B
LSEGS = (8, 19, 64)
ROWS = 13                                # window rows of a merged job's table
HEAVY_PARTS = rc.HEAVY_PARTS
REDUCE_G = 8                             # buckets per reduction lane, the prover's own
GUARDS = 8
FILL_WORD = 0xA5A5A5A5


def _acc_threads():
    text = open(os.path.join(fc.ROOT, "groth16_amd", "csrc", "acc_store.hpp")).read()
    (v,) = re.findall(r"static constexpr int ACC_THREADS = (\d+);", text)
    return int(v)


ACC_THREADS = _acc_threads()
TASKS_PER_WG = {False: ACC_THREADS, True: ACC_THREADS // 2}   # a task is one lane (G1) or one lane pair (G2)

# the table every job starts from, as multiples of the generator: P twice, 2P, Q, the identity base (0, 0), then fillers
K_P, K_Q = 3, 10
TABLE = (K_P, K_P, 2 * K_P, K_Q, 0, 7, 11, 13, 17, 19, 23)
I_P, I_P2, I_2P, I_Q, I_O, I_FILL = 0, 1, 2, 3, 4, 5


class PassModel:
    def __init__(self, curve, g2):
        self.curve, self.g2 = curve, g2
        self.m = rc.model(curve, g2)
        self.G, self.r = self.m.G, self.m.cp.r
        self.gen = self.m.pts[0]
        self._pts = {}

    def point(self, k):
        """k G as an affine point (None: the identity), k a signed integer"""
        k %= self.r
        if k > self.r // 2:
            P = self.point(self.r - k)
            return self.G.neg(P)
        if k not in self._pts:
            self._pts[k] = self.G.mul(self.gen, k) if k else None
        return self._pts[k]


@functools.lru_cache(maxsize=None)
def model(curve, g2):
    return PassModel(curve, g2)


def tag_add(acc, k, r):
    """what the addition acc += k G is, as reduce_cases.Model.add names it"""
    if k % r == 0:
        return "skip"
    if acc % r == 0:
        return "copy"
    if (acc - k) % r == 0:
        return "dbl"
    if (acc + k) % r == 0:
        return "cancel"
    return "hot"


class Job:
    """One job of a lab call: table, shift, base_count, the entries bucket by bucket; finish() derives everything the test compares."""

    def __init__(self, pm, merged, lseg, name, table=TABLE, shift=0, base_count=None):
        self.pm, self.merged, self.lseg, self.name = pm, merged, lseg, name
        self.rows = ROWS if merged else 1
        self.table = list(table)                 # row 0, as multiples of G; row j holds 2^(C_BITS j) times these
        self.base_count = len(self.table) if base_count is None else base_count
        self.shift = shift
        self.buckets = [[] for _ in range(M)]    # entry words in walk order
        self.named = {}                          # case name -> bucket
        self.seen = set()                        # events asserted with the model
        self.next, self.pos = 0, 0

    # ---- entry words ----------------------------------------------------------------------------------------------------------------
    def word(self, idx, neg=False, row=0):
        """the entry that addresses table index idx (after shift) of window row `row`"""
        pt = idx - self.shift
        assert 0 <= pt < (1 << 26) and 0 <= row < self.rows
        return pt | (row << 26 if self.merged else 0) | (int(neg) << 31)

    def decode(self, v):
        """(signed multiple of G, or None for a skipped entry) by the rule of the kernel's documentation, msm.hip `decode`"""
        pt = v & 0x3FFFFFF if self.merged else v & 0x7FFFFFFF
        row = (v >> 26) & 31 if self.merged else 0
        idx = pt + self.shift
        if not 0 <= idx < self.base_count:
            return None
        k = self.table[idx] << (C_BITS * row)
        if k == 0:
            return None                          # the identity base
        return -k if v >> 31 else k

    def fill(self, rng, n):
        rows = min(self.rows, 2)
        return [self.word(rng.randrange(I_FILL, min(len(self.table), self.base_count)), rng.randrange(2) == 1, rng.randrange(rows)) for _ in range(n)]

    # ---- layout ---------------------------------------------------------------------------------------------------------------------
    def skip(self, k):
        self.next += k

    def bucket(self, entries, name=None):
        b = self.next
        assert b < M and entries, "out of buckets"
        self.buckets[b] = list(entries)
        self.pos += len(entries)
        self.next += 1
        if name:
            assert name not in self.named
            self.named[name] = b
        return b

    def pad_to(self, rng, rem):
        """filler entries in a bucket of their own until the next bucket starts at position rem mod lseg"""
        need = (rem - self.pos) % self.lseg
        if need:
            self.bucket(self.fill(rng, need))

    # ---- the model ------------------------------------------------------------------------------------------------------------------
    def finish(self):
        L, r = self.lseg, self.pm.r
        self.counts = [len(q) for q in self.buckets]
        self.sorted = [v for q in self.buckets for v in q]
        self.S = len(self.sorted)
        self.offsets = [0]
        for n in self.counts:
            self.offsets.append(self.offsets[-1] + n)
        self.nparts, self.task_off, self.heavy = [], [0], set()
        self.shares = {}       # (bucket, segment) -> [signed multiple or None per entry]
        self.expected = []     # per slot: the share's sum as a multiple of G
        self.share_tags = {}   # (bucket, segment) -> tags of the walk's additions
        self.sums = []
        for b in range(M):
            lo, hi = self.offsets[b], self.offsets[b + 1]
            np_ = (hi - 1) // L - lo // L + 1 if hi > lo else 0
            self.nparts.append(np_)
            self.task_off.append(self.task_off[-1] + np_)
            if np_ > HEAVY_PARTS:
                self.heavy.add(b)
            total = 0
            for t in range(lo // L, lo // L + np_):
                ks = [self.decode(v) for v in self.sorted[max(lo, t * L):min(hi, (t + 1) * L)]]
                assert ks
                acc, tags = 0, []
                for k in ks:
                    tags.append(tag_add(acc, k or 0, r))
                    acc += k or 0
                self.shares[(b, t)], self.share_tags[(b, t)] = ks, tags
                self.expected.append(acc)
                total += acc
            self.sums.append(total)
        assert len(self.expected) == self.task_off[M] <= (self.S + L - 1) // L + M
        if self.merged:
            self.total = sum((k + 1) * S for k, S in enumerate(self.sums))
        else:
            self.total = sum((sum((b + 1) * self.sums[w * B + b] for b in range(B))) << (C_BITS * w) for w in range(GROUPS))
        self.skipped = sum(k is None for ks in self.shares.values() for k in ks)
        return self

    # ---- what the generators assert -------------------------------------------------------------------------------------------------
    def segs(self, b):
        lo = self.offsets[b] // self.lseg
        return list(range(lo, lo + self.nparts[b]))

    def tags(self, b):
        return [self.share_tags[(b, t)] for t in self.segs(b)]

    def combine_tags(self, b):
        """bucket_combine_kernel adds the bucket's records 1.. into record 0"""
        first = self.task_off[b]
        acc, tags = self.expected[first], []
        for k in self.expected[first + 1:self.task_off[b + 1]]:
            tags.append(tag_add(acc, k, self.pm.r))
            acc += k
        return tags

    def flushed_in_loop(self, b):
        """the bucket's last share is stored by the flush inside the loop (another bucket follows in the same segment), not by the one
        after it"""
        hi = self.offsets[b + 1]
        return hi % self.lseg != 0 and hi < self.S

    def table_points(self):
        """[rows * base_count] affine points (None: the identity), row j = 2^(C_BITS j) times row 0"""
        return [self.pm.point(k << (C_BITS * j)) for j in range(self.rows) for k in self.table[:self.base_count]]


# ---- the jobs ------------------------------------------------------------------------------------------------------------------------
def _boundaries(job, rng):
    L = job.lseg
    P, Q = job.word(I_P), job.word(I_Q)
    job.skip(1)
    b_exact = job.bucket(job.fill(rng, L), "a bucket of exactly lseg entries on a segment boundary")
    b_first = job.bucket([P], "a one-entry bucket, first entry of a segment")
    job.bucket(job.fill(rng, L - 2))
    b_last = job.bucket([Q], "a one-entry bucket, last entry of a segment")
    job.bucket(job.fill(rng, L // 2))
    b_two = job.bucket(job.fill(rng, L), "a bucket from mid-segment over 2 segments")
    b_three = job.bucket(job.fill(rng, 2 * L), "a bucket from mid-segment over 3 segments")
    job.pad_to(rng, 0)
    run = [job.bucket(job.fill(rng, 1), "before a run of 1 empty bucket")]
    job.skip(1)
    run.append(job.bucket(job.fill(rng, 1), "before a run of 2 empty buckets"))
    job.skip(2)
    run.append(job.bucket(job.fill(rng, 1), "before a run of 31 empty buckets across the group boundary"))
    job.skip(31)
    run.append(job.bucket(job.fill(rng, 2), "after a run of 31 empty buckets"))
    job.finish()
    o, n = job.offsets, job.nparts
    assert job.counts[0] == 0 and job.counts[M - 1] == 0
    assert o[b_exact] % L == 0 and job.counts[b_exact] == L and n[b_exact] == 1
    assert o[b_first] % L == 0 and job.counts[b_first] == 1
    assert o[b_last] % L == L - 1 and job.counts[b_last] == 1
    assert o[b_two] % L and n[b_two] == 2 and o[b_three] % L and n[b_three] == 3
    assert len({job.segs(b)[0] for b in run}) == 1 and all(n[b] == 1 for b in run)          # one segment holds all four
    assert [run[i + 1] - run[i] - 1 for i in range(3)] == [1, 2, 31] and run[2] < B <= run[3]
    assert all(job.counts[b] == 0 for b in range(run[2] + 1, run[3]))
    job.seen.update(["bucket 0 empty", "bucket M-1 empty", "runs of 1, 2 and 31 empty buckets inside one segment", "an empty run across the group boundary"])


def _last_bucket_only(job, rng):
    job.skip(M - 1)
    b = job.bucket(job.fill(rng, 2 * job.lseg + 3), "buckets 0..M-2 empty")
    job.finish()
    assert b == M - 1 and job.nparts[b] == 3 and job.task_off[b] == 0
    job.seen.add("buckets 0..M-2 empty")


def _segments(job, rng):
    L = job.lseg
    job.skip(3)
    n1 = job.bucket(job.fill(rng, L + 3), "the left neighbour of a bucket of HEAVY_PARTS segments")
    h0 = job.bucket(job.fill(rng, (L - 3) + (HEAVY_PARTS - 2) * L + 2), "a bucket of HEAVY_PARTS segments")
    n2 = job.bucket(job.fill(rng, 1), "between the buckets of HEAVY_PARTS and HEAVY_PARTS + 1 segments")
    job.skip(2)
    h1 = job.bucket(job.fill(rng, (L - 3) + (HEAVY_PARTS - 1) * L + 2), "a bucket of HEAVY_PARTS + 1 segments")
    n3 = job.bucket(job.fill(rng, 4), "the right neighbour of a bucket of HEAVY_PARTS + 1 segments")
    job.finish()
    assert job.nparts[h0] == HEAVY_PARTS and job.nparts[h1] == HEAVY_PARTS + 1 and job.heavy == {h1}
    assert job.segs(n1)[-1] == job.segs(h0)[0] and job.segs(h0)[-1] == job.segs(n2)[0] == job.segs(h1)[0] and job.segs(h1)[-1] == job.segs(n3)[0]
    job.seen.update(["HEAVY_PARTS segments: not heavy", "HEAVY_PARTS + 1 segments: heavy", "neighbours share the first and the last segment"])


def _collisions(job, rng):
    """shift = -1 here: word() adds one to every index, and the raw point index 0 is moved out of range"""
    L = job.lseg
    assert job.shift == -1
    P, P2, nP, nP2, dP, ndP, Q, O = (job.word(I_P), job.word(I_P2), job.word(I_P, True), job.word(I_P2, True), job.word(I_2P), job.word(I_2P, True),
                                     job.word(I_Q), job.word(I_O))
    OUT = 0 | (1 << 31)      # point index 0 + shift = -1, with the sign bit for good measure
    F = lambda n: job.fill(rng, n)   # noqa: E731
    job.skip(2)
    job.bucket(F(L - 2))
    a = job.bucket([P, nP2], "[P, -P] as a whole share, stored by the flush after the loop")
    b = job.bucket([dP, nP, nP2], "[2P, -P, -P]: a share that cancels just before the flush inside the loop")
    c = job.bucket([P, nP2, Q], "[P, -P, Q]")
    d = job.bucket([P, P2], "[P, P]")
    e = job.bucket([P2, P, ndP], "[P, P, -2P]")
    job.pad_to(rng, L - 1)
    f = job.bucket([P, nP], "P last in segment t, -P first in segment t + 1")
    job.pad_to(rng, L - 1)
    g = job.bucket([P, P2], "P last in segment t, P first in segment t + 1")
    job.skip(1)
    h = job.bucket([O, OUT, O], "a share of skipped entries only")
    job.pad_to(rng, 0)
    i = job.bucket([OUT, P, Q], "a skipped entry first in a bucket")
    j = job.bucket([P, Q, O], "a skipped entry last in a bucket")
    job.pad_to(rng, 0)
    k = job.bucket([P, OUT, nP2], "a skipped entry between P and -P")
    job.pad_to(rng, L - 1)
    l = job.bucket([O, P], "a skipped share last in segment t, P first in segment t + 1")
    job.bucket(F(3))
    job.finish()
    T, kP, kQ = job.tags, K_P, K_Q
    assert T(a) == [["copy", "cancel"]] and job.offsets[a + 1] % L == 0 and not job.flushed_in_loop(a)
    assert T(b) == [["copy", "hot", "cancel"]] and job.flushed_in_loop(b)
    assert T(c) == [["copy", "cancel", "copy"]] and job.sums[c] == kQ
    assert T(d) == [["copy", "dbl"]] and job.sums[d] == 2 * kP
    assert T(e) == [["copy", "dbl", "cancel"]] and job.sums[e] == 0
    assert T(f) == [["copy"], ["copy"]] and job.combine_tags(f) == ["cancel"] and job.sums[f] == 0
    assert T(g) == [["copy"], ["copy"]] and job.combine_tags(g) == ["dbl"] and job.sums[g] == 2 * kP
    assert T(h) == [["skip", "skip", "skip"]] and job.shares[(h, job.segs(h)[0])] == [None] * 3
    assert T(i) == [["skip", "copy", "hot"]] and T(j) == [["copy", "hot", "skip"]] and job.sums[i] == job.sums[j] == kP + kQ
    assert T(k) == [["copy", "skip", "cancel"]] and job.sums[k] == 0
    assert T(l) == [["skip"], ["copy"]] and job.combine_tags(l) == ["copy"]
    for x in (a, b, e, h, k):
        assert job.expected[job.task_off[x]] == 0            # an identity record that the walk must WRITE
    job.seen.update(["[P, -P]", "[P, -P] before the flush inside the loop", "[P, -P, Q]", "[P, P]", "[P, P, -2P]", "the combine cancels", "the combine doubles",
                     "a share of skipped entries only", "skipped first", "skipped last", "skipped between P and -P"])


def _spread(job, rng, S, lo_idx=0):
    """S entries over random buckets, indices over the whole table (whatever shift and base_count then make of them)"""
    per = [0] * M
    for _ in range(S):
        per[rng.randrange(M)] += 1
    rows = min(job.rows, 2)
    n = len(job.table) - lo_idx
    idx = [lo_idx + i % n for i in range(S)]       # every index at least once where S allows
    rng.shuffle(idx)
    for b in range(M):
        if per[b]:
            job.next = b
            job.bucket([idx.pop() | (rng.randrange(rows) << 26 if job.merged else 0) | (rng.randrange(2) << 31) for _ in range(per[b])])
    return job.finish()


def _shift(job, rng):
    """raw point indices 0 .. len(table) - 1: shift = -1 moves index 0 out of range, shift = +1 the last one, shift = -n all of them"""
    n = len(job.table)
    _spread(job, rng, 3 * job.lseg + 5)
    valid = sum(k is not None for ks in job.shares.values() for k in ks)
    moved_out = [v for v in job.sorted if not 0 <= (v & (0x3FFFFFF if job.merged else 0x7FFFFFFF)) + job.shift < job.base_count]
    assert moved_out and all(job.decode(v) is None for v in moved_out)
    if job.shift == -n:
        job.seen.add("shift = -n: every entry skipped")
        assert valid == 0 and all(k == 0 for k in job.expected) and job.expected
    else:
        assert valid and job.skipped
        job.seen.add("shift = %+d: some entries skipped, some not" % job.shift)


def _base_count(job, rng):
    _spread(job, rng, 3 * job.lseg + 5)
    assert job.base_count < len(job.table)
    beyond = [v for v in job.sorted if (v & 0x3FFFFFF) >= job.base_count]
    assert beyond and all(job.decode(v) is None for v in beyond) and any(job.decode(v) for v in job.sorted)
    job.seen.add("base_count below the largest index")


def _rows(job, rng):
    """merged: every window row with every table index, the sign bit on the last row's last point"""
    assert job.merged
    words = [job.word(i, (i + j) % 3 == 0, j) for j in range(ROWS) for i in range(job.base_count)]
    last = job.word(job.base_count - 1, True, ROWS - 1)
    words.append(last)
    rng.shuffle(words)
    at = 0
    job.skip(5)
    while at < len(words):
        n = rng.randrange(2, 9)
        job.bucket(words[at:at + n])
        job.skip(rng.randrange(2))
        at += n
    job.finish()
    assert last == (job.base_count - 1) | (12 << 26) | (1 << 31) and job.decode(last) == -(job.table[job.base_count - 1] << (C_BITS * 12))
    assert {(v >> 26) & 31 for v in job.sorted} == set(range(ROWS))
    job.seen.add("every row 0..12; sign bit on row 12 at index base_count - 1")


def _bit26(job, rng):
    """per-window: the point index takes bits 0..30, so an index with bit 26 or above set is a large index, not a window tag"""
    assert not job.merged
    P = job.word(I_P)
    high = [(1 << 26) | I_P, (1 << 27) | I_Q, (1 << 30) | I_P, (5 << 26) | I_2P | (1 << 31), 0x7FFFFFFF]
    job.skip(4)
    job.bucket([P, high[0], high[1]], "indices with bit 26 and bit 27 set after P")
    job.bucket([high[2], P], "an index with bit 30 set first in a bucket")
    job.bucket([high[3], high[4]], "a share of high indices only")
    job.bucket(job.fill(rng, job.lseg))
    job.finish()
    assert all(job.decode(v) is None for v in high) and job.sums[4] == job.sums[5] == K_P and job.sums[6] == 0
    job.seen.add("bit 26 and above set: skipped")


def _size(S):
    def make(job, rng):
        _spread(job, rng, S(job), lo_idx=I_FILL)
        assert job.S == S(job)
        if job.S > job.lseg:
            assert job.S % job.lseg == 1       # the last segment holds one entry
        tasks = (job.S + job.lseg - 1) // job.lseg
        job.seen.add("S = %d: %d tasks, %d in the last workgroup" % (job.S, tasks, tasks % TASKS_PER_WG[job.pm.g2]))
    return make


ALT_TABLE = (29, 0, 31, 37, 41, K_P, 43)

# name -> (generator, Job keywords, which plans)
JOBS = {
    "boundaries": (_boundaries, {}, "both"),
    "last_bucket_only": (_last_bucket_only, {}, "both"),
    "segments": (_segments, {}, "both"),
    "collisions": (_collisions, {"shift": -1}, "both"),
    "shift_minus_1": (_shift, {"shift": -1}, "both"),
    "shift_plus_1": (_shift, {"shift": 1, "table": ALT_TABLE}, "both"),
    "shift_minus_n": (_shift, {"shift": -len(TABLE)}, "both"),
    "base_count_below": (_base_count, {"base_count": 6}, "both"),
    "rows": (_rows, {"base_count": 7}, "merged"),
    "bit26": (_bit26, {}, "per_window"),
    "S0": (_size(lambda job: 0), {}, "both"),
    "S1": (_size(lambda job: 1), {}, "both"),
    "S_lseg": (_size(lambda job: job.lseg), {}, "both"),
    "S_lseg_plus_1": (_size(lambda job: job.lseg + 1), {"table": ALT_TABLE}, "both"),
    "S_second_workgroup": (_size(lambda job: TASKS_PER_WG[job.pm.g2] * job.lseg + 1), {}, "both"),
}
# one launch of four: different S (one of them 0), different tables, shifts and base_counts
BATCH = ("S_lseg_plus_1", "S0", "collisions", "base_count_below")


def job_names(merged):
    return [n for n, (_, _, plans) in JOBS.items() if plans in ("both", "merged" if merged else "per_window")]


@functools.lru_cache(maxsize=None)
def job(curve, g2, merged, lseg, name):
    make, kw, _ = JOBS[name]
    j = Job(model(curve, g2), merged, lseg, name, **kw)
    make(j, random.Random("pass/%s/%d/%d/%d/%s" % (curve, g2, merged, lseg, name)))
    assert j.S == sum(j.counts) <= 1 << 16
    return j


def configs():
    return [(curve, g2, merged, lseg) for curve in ("bls12_381", "bn254") for g2 in (False, True) for merged in (False, True) for lseg in LSEGS]


def config_id(curve, g2, merged, lseg):
    return "%s-%s-%s-L%d" % (curve, "g2" if g2 else "g1", "merged" if merged else "per_window", lseg)


# ---- the sort lab: signed digits -----------------------------------------------------------------------------------------------------
def digits(s, c, W):
    """the signed-digit decomposition of s over W windows of c bits, by carries from the bottom; checked on its own"""
    half, full = 1 << (c - 1), 1 << c
    out, rest = [], s
    for _ in range(W):
        d = rest & (full - 1)
        rest >>= c
        if d >= half:
            d -= full
            rest += 1
        out.append(d)
    assert rest == 0, "W = %d windows of %d bits do not hold %d" % (W, c, s)
    assert sum(d << (c * w) for w, d in enumerate(out)) == s and all(-half <= d < half for d in out)
    return out


def value(ds, c):
    return sum(d << (c * w) for w, d in enumerate(ds))


def digit_edge_scalars(r, c, W, seed=5):
    """scalars in [0, r) that hold the digits a random scalar practically never does; vectors whose value leaves [0, r) are dropped"""
    half = 1 << (c - 1)
    hi, lo = half - 1, -half
    vecs = []
    top_max = max(d for d in (digits(r - 1, c, W)[W - 1] - 1, 0))
    for top in sorted({0, 1, top_max}):
        vecs.append([hi] * (W - 1) + [top])                                   # every digit 2^(c-1) - 1 below a top digit under r
    for w in range(W - 1):
        v = [0] * W
        v[w], v[w + 1] = lo, 1
        vecs.append(v)                                                        # one digit -2^(c-1) under a +1, at every position
    vecs.append([hi if w % 2 == 0 else lo for w in range(W - 1)] + [1])       # alternating extremes
    vecs.append([lo if w % 2 == 0 else hi for w in range(W - 1)] + [1])
    for w in range(W):
        for d in (1, hi, -1, lo) + ((top_max,) if w == W - 1 else ()):
            v = [0] * W
            v[w] = d
            vecs.append(v)                                                    # all digits zero but one, at every position
    out = [value(v, c) for v in vecs]
    out += [0, 1, r - 1, (r - 1) // 2, (r + 1) // 2]
    # the largest s < r whose top raw window (the bits from c (W' - 1) up, W' the number of windows r itself needs) is all ones
    Wr = (r.bit_length() + c - 1) // c
    top_bits = r.bit_length() - c * (Wr - 1)
    for ones in range(top_bits, 0, -1):
        s = (((1 << ones) - 1) << (c * (Wr - 1))) | ((1 << (c * (Wr - 1))) - 1)
        if s < r:
            out.append(s)
            break
    rng = random.Random("digits/%d/%d" % (c, seed))
    out += [rng.randrange(r) for _ in range(64)]
    keep = []
    for s in out:
        if 0 <= s < r and s not in keep:
            keep.append(s)
    return keep


def sort_scalars(r, c, W, n):
    """n scalars for a sort-lab call: the digit edges first (cycled when n is larger), cut to n"""
    pool = digit_edge_scalars(r, c, W)
    rng = random.Random("sort/%d/%d" % (c, n))
    picks = list(pool)
    rng.shuffle(picks)
    return [picks[i % len(picks)] for i in range(n)]


def sort_model(scalars, c, W, merged, B_, groups, lseg, shard_n=1, shard_r=0):
    """({bucket: sorted list of (point, window, sign)} for the non-empty buckets, offsets, task_off, the heavy set) by the rules at the top"""
    import numpy as np

    Mb = B_ * groups
    buckets = {}
    for i, s in enumerate(scalars):
        for w, d in enumerate(digits(s, c, W)):
            if d == 0:
                continue
            key = abs(d) - 1
            if merged:
                if key % shard_n != shard_r:
                    continue
                b = key // shard_n
            else:
                b = w * B_ + key
            assert b < Mb
            buckets.setdefault(b, []).append((i, w, int(d < 0)))
    counts = np.zeros(Mb, dtype=np.int64)
    for b, q in buckets.items():
        counts[b] = len(q)
        q.sort()
    offsets = np.concatenate([[0], np.cumsum(counts)])
    lo, hi = offsets[:-1], offsets[1:]
    nparts = np.where(hi > lo, (hi - 1) // lseg - lo // lseg + 1, 0)
    task_off = np.concatenate([[0], np.cumsum(nparts)])
    heavy = {int(b) for b in np.nonzero(nparts > HEAVY_PARTS)[0]}
    return buckets, offsets, task_off, heavy
