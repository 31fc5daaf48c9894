"""Crafted partial sums for the reduction lab (g16_dev_msm_reduce_lab) and its batch form (g16_dev_msm_reduce_batch_lab: BATCHES,
batch_conditions) and the model of what the reductions make of them (TEST INFRASTRUCTURE).

The lab runs the prover's own reduction -- heavy_reduce_kernel, bucket_combine_kernel, bucket_reduce_kernel, window_reduce_kernel and
the host fold -- on partial sums the caller wrote, so a test can place what whole MSMs on random data never reach: equal and opposite
points inside one bucket's list of partial sums, in the running sums of a chunk of buckets, and in the trees over tasks and chunks.

A partial sum is an AccRaw record (fp30.hpp): (x, y, zz, zzz) = (X z^2, Y z^3, z^2, z^3) in the R' Montgomery domain as raw lazy limbs.
The representatives are the ones the producers promise (the comments at Acc30 and AccParked::gather): x < 7.5 p, so r + kx p for
kx = 0..6; y < 3.5 p parked and 4 p - y out of gather(), so r + ky p for ky = 0..3; zz, zzz < 1.8 p, so r, and r + p where that stays
below 1.8 p.  The identity is an all-zero record (gather_as_parked zeroes every coordinate; readers look at zz alone).

The model is pymodel's group law on affine points.  It replays the ORDER in which each kernel adds -- a lane's left fold, a task's
strided run, the trees -- only to name what every addition is (a copy into an identity, a doubling, a cancellation, a plain
addition), so that a scenario can assert, with the model alone, that the collision it is named after really happens.  The expected
values do not depend on that order: a bucket's sum, and  sum_w 2^(c w) sum_b (b + 1) S_(w,b)  (per-window fold) or
sum_k (k + 1) S_k over the bucket key k = group * B + b  (merged fold)."""
import collections
import functools
import os
import random
import re
import sys

import fp30_cases as fc

sys.path.insert(0, os.path.join(fc.ROOT, "oracle"))
import pymodel  # noqa: E402

C_BITS, GROUPS = 6, 2                   # 32 buckets per group, two groups
B = 1 << (C_BITS - 1)
# The kernels' launch shapes.  The expected values do not depend on them; the replayed add order -- and with it the generator's claim
# that a named doubling or cancellation happens in a tree or a task's run -- does.  They are read from the sources, so a change of
# HEAVY_PARTS, HEAVY_THREADS or WIN_THREADS moves the crafted positions with it instead of leaving the tests green on other additions.
def _source_constant(path, name):
    text = open(os.path.join(fc.ROOT, "groth16_amd", "csrc", path)).read()
    (v,) = re.findall(r"static constexpr (?:int|uint32_t) %s = (\d+);" % name, text)
    return int(v)


HEAVY_PARTS = _source_constant("internal.hpp", "HEAVY_PARTS")        # a bucket with more partial sums goes to heavy_reduce_kernel
HEAVY_THREADS = _source_constant("msm.hip", "HEAVY_THREADS")
WIN_THREADS = _source_constant("msm.hip", "WIN_THREADS")
HEAVY_TASKS = {False: HEAVY_THREADS, True: HEAVY_THREADS // 2}   # a task is one lane (G1) or one lane pair (G2)
WIN_TASKS = {False: WIN_THREADS, True: WIN_THREADS // 2}
CHUNKS = (8, 16, 32)                    # buckets per reduction lane: 4 and 2 chunks per group (bit planes live), and the whole group
SCENARIOS = ("combine", "chains")
# The batch lab (g16_dev_msm_reduce_batch_lab, G1) reduces up to four jobs in one launch per kernel; a job is a scenario.  "complement",
# "empty" and "single" exist for it: what tells the jobs of a batch apart (batch_conditions).
BATCH_SCENARIOS = SCENARIOS + ("complement", "empty", "single")
BATCHES = (
    ("combine", "chains", "complement", "empty"),
    ("empty", "complement", "chains", "combine"),       # the reverse
    ("complement", "empty", "chains", "combine"),       # complement first, combine last
    ("complement", "combine"),
    ("chains", "complement", "combine"),
    ("combine", "combine"),                             # two separate copies: same offsets and lists, other buffers
    ("single",),
)
# early mode: the jobs of the subset have their first stage in one launch (msm_heavy_reduce_batch), the others alone; {0, 1, 2} is what
# the single-GPU proof does with l, a, b_g1 before h
EARLY_SUBSETS = {4: ((0, 1, 2), (0,), (1, 2)), 3: ((1, 2),)}


Rep = collections.namedtuple("Rep", "point kx ky")   # a partial sum with chosen representatives: x + kx p, y + ky p per component


def _rep(q):
    return q if isinstance(q, Rep) else Rep(q, None, None)


class Model:
    def __init__(self, curve, g2):
        self.curve, self.g2 = curve, g2
        self.cp = pymodel.CURVES[curve]
        self.G = pymodel.groups(self.cp)[1 if g2 else 0]
        self.F = self.G.F
        self.f = fc.Field(curve, "fq")
        self.C = 2 if g2 else 1
        self.words = 4 * self.C * self.f.NL
        gen = self.cp.g2 if g2 else self.cp.g1
        self.pts = [gen]
        for _ in range(95):
            self.pts.append(self.G.add(self.pts[-1], gen))

    def comps(self, e):
        return list(e) if self.g2 else [e]

    def elem(self, c):
        return (c[0], c[1]) if self.g2 else c[0]

    # ---- records ------------------------------------------------------------------------------------------------------------------
    def record(self, P, rng, kx=None, ky=None):
        """P as a lazy record with a random scale z; kx / ky: the representative's multiple of p per component (None: random)"""
        f, p, F, C = self.f, self.f.p, self.F, self.C
        if P is None:
            return [0] * self.words
        z = self.elem([rng.randrange(1, p) for _ in range(C)])
        zz = F.sqr(z)
        zzz = F.mul(zz, z)
        kx = [rng.randrange(7) for _ in range(C)] if kx is None else [kx] * C
        ky = [rng.randrange(4) for _ in range(C)] if ky is None else [ky] * C
        out = []
        for e, ks in ((F.mul(P[0], zz), kx), (F.mul(P[1], zzz), ky), (zz, None), (zzz, None)):
            for i, c in enumerate(self.comps(e)):
                r = c * f.R % p
                if ks is None:   # zz, zzz < 1.8 p
                    k = 1 if (5 * (r + p) < 9 * p and rng.randrange(2)) else 0
                else:
                    k = ks[i]
                out += f.limbs(r + k * p)
        return out

    def decode(self, words):
        """a record's point: None for the identity (all-zero zz), else canonical affine"""
        f, p, F, C, NL = self.f, self.f.p, self.F, self.C, self.f.NL
        v = [[f.value([int(x) for x in words[(e * C + c) * NL:(e * C + c + 1) * NL]]) for c in range(C)] for e in range(4)]
        if not any(v[2]):
            return None
        rinv = pow(f.R, -1, p)
        x, y, zz, zzz = [self.elem([c * rinv % p for c in e]) for e in v]
        return (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))

    # ---- the additions, named -------------------------------------------------------------------------------------------------------
    def add(self, a, b, tags=None):
        """a += b as acc_add_streamed sees it"""
        if b is None:
            tag = "skip"
        elif a is None:
            tag = "copy"
        elif a == b:
            tag = "dbl"
        elif a == self.G.neg(b):
            tag = "cancel"
        else:
            tag = "hot"
        if tags is not None:
            tags.append(tag)
        return self.G.add(a, b)

    def fold_list(self, parts):
        """bucket_combine_kernel: one task adds partials 1.. into partial 0"""
        tags, acc = [], parts[0]
        for q in parts[1:]:
            acc = self.add(acc, q, tags)
        return acc, tags

    def tree(self, vals, tasks):
        """the LDS trees of heavy_reduce_kernel / window_reduce_kernel over per-task sums"""
        sh = list(vals) + [None] * (tasks - len(vals))
        tags = []
        d = tasks // 2
        while d > 0:
            for t in range(d):
                sh[t] = self.add(sh[t], sh[t + d], tags)
            d //= 2
        return sh[0], tags

    def heavy(self, parts):
        """heavy_reduce_kernel: task t adds partials t, t + TASKS, ... from the identity, then the tree"""
        T = HEAVY_TASKS[self.g2]
        sums, runs = [], []
        for t in range(min(T, len(parts))):
            tags, acc = [], None
            for q in parts[t::T]:
                acc = self.add(acc, q, tags)
            sums.append(acc)
            runs.append(tags)
        total, tags = self.tree(sums, T)
        return total, runs, sums, tags

    def chunk(self, sums):
        """bucket_reduce_kernel over one chunk (sums in ascending bucket order): (run, tot, tags of `run +=`, tags of `tot +=`)"""
        run = tot = None
        rt, tt = [], []
        for S in reversed(sums):
            run = self.add(run, S, rt)
            tot = self.add(tot, run, tt)
        return run, tot, rt, tt


class Scenario:
    """nparts [GROUPS * B], records [sum(nparts)][words], sums [GROUPS * B] (the model's bucket sums), named {bucket: name}"""

    def __init__(self, m, merged, chunk, name):
        self.m, self.merged, self.chunk, self.name = m, merged, chunk, name
        self.parts = [[] for _ in range(GROUPS * B)]    # per bucket: [(point or None, kx, ky)]
        self.named = {}
        self.seen = set()                               # collisions asserted with the model, "<kernel>: <what>"

    def put(self, b, parts, name=None):
        assert not self.parts[b], "bucket %d is taken" % b
        self.parts[b] = [_rep(q) for q in parts]
        if name:
            self.named[b] = name

    def finish(self, rng):
        m = self.m
        self.nparts = [len(q) for q in self.parts]
        self.records = [m.record(P, rng, kx, ky) for q in self.parts for P, kx, ky in q]
        self.sums = []
        for q in self.parts:
            acc = None
            for P, _, _ in q:
                acc = m.G.add(acc, P)
            self.sums.append(acc)
        G = m.G
        total = None
        if self.merged:
            for k, S in enumerate(self.sums):
                total = G.add(total, G.mul(S, k + 1))
        else:
            for w in range(GROUPS):
                T = None
                for b in range(B):
                    T = G.add(T, G.mul(self.sums[w * B + b], b + 1))
                total = G.add(total, G.mul(T, 1 << (C_BITS * w)))
        self.total = total
        return self


def _combine(sc, rng):
    """group 0: every crafted list of partial sums in a bucket of its own, random buckets beside them; group 1: all empty"""
    m, G = sc.m, sc.m.G
    pts = list(m.pts)
    rng.shuffle(pts)
    P, Q, S = pts[0], pts[1], pts[2]
    neg = G.neg
    O = None
    lists = [
        ("[O, P, -P]", [O, P, neg(P)], ["copy", "cancel"]),
        ("[O, O, P, -P]", [O, O, P, neg(P)], ["skip", "copy", "cancel"]),
        ("[O, P, -P, Q]", [O, P, neg(P), Q], ["copy", "cancel", "copy"]),
        ("[P, -P]", [P, neg(P)], ["cancel"]),
        ("[P, -P, P]", [P, neg(P), P], ["cancel", "copy"]),
        ("[P, P] with two scales", [Rep(P, 6, 3), Rep(P, 0, 0)], ["dbl"]),
        ("[P, P, -2P]", [P, P, neg(G.add(P, P))], ["dbl", "cancel"]),
        ("[O, O, O]", [O, O, O], ["skip", "skip"]),
        ("[O, P]", [O, P], ["copy"]),
        ("[P, O]", [P, O], ["skip"]),
        ("[P, Q, S]", [Rep(P, 6, 0), Rep(Q, 0, 3), Rep(S, 3, 2)], ["hot", "hot"]),
    ]
    free = list(range(B))
    rng.shuffle(free)
    for name, parts, want_tags in lists:
        _, tags = m.fold_list([_rep(q).point for q in parts])
        assert tags == want_tags, (name, tags)
        sc.put(free.pop(), parts, "bucket_combine_kernel " + name)
        sc.seen.add("bucket_combine_kernel: " + name)
    # the last count bucket_combine_kernel takes and the first that heavy_reduce_kernel takes, identities mixed in
    for n, kernel in ((HEAVY_PARTS, "bucket_combine_kernel"), (HEAVY_PARTS + 1, "heavy_reduce_kernel")):
        parts = [None if i % 5 == 2 else pts[3 + (i * 7 + n) % 60] for i in range(n)]
        parts[0] = None if n == HEAVY_PARTS else parts[0]
        sc.put(free.pop(), parts, "%s %d partial sums" % (kernel, n))
    # a heavy bucket with more partial sums than the kernel has tasks: task 0's strided run is [P, -P], tasks 1 and 1 + T/2 end with
    # equal sums (the tree doubles), tasks 2 and 2 + T/2 with opposite sums (the tree cancels)
    T = HEAVY_TASKS[m.g2]
    n = T + 8
    parts = [None] * n
    for i in range(n):
        if i % 3 != 1:
            parts[i] = pts[8 + (i * 11) % 80]
    A, Bp, Cp, D = pts[90], pts[91], pts[92], pts[93]
    parts[0], parts[T], parts[T // 2] = A, neg(A), Q   # (task 0 ends as the identity and takes task T/2's sum in the tree)
    parts[1], parts[1 + T] = Bp, Cp
    parts[1 + T // 2] = G.add(Bp, Cp)
    parts[2], parts[2 + T] = D, Bp
    parts[2 + T // 2] = neg(G.add(D, Bp))
    total, runs, sums, tags = m.heavy(parts)
    assert runs[0] == ["copy", "cancel"] and sums[0] is None, runs[0]
    assert runs[1] == ["copy", "hot"] and runs[2] == ["copy", "hot"], (runs[1], runs[2])
    assert tags[0] == "copy" and tags[1] == "dbl" and tags[2] == "cancel", tags[:3]   # first tree level: task t += task t + T/2
    sc.put(free.pop(), parts, "heavy_reduce_kernel more partial sums than tasks: a run [P, -P], a doubling and a cancellation in the tree")
    sc.seen.update(["heavy_reduce_kernel: a task's run is [P, -P]", "heavy_reduce_kernel: the tree doubles", "heavy_reduce_kernel: the tree cancels"])
    # the rest of group 0: empty, or random lists with identities
    for b in free:
        k = rng.randrange(5)
        if k:
            sc.put(b, [None if rng.randrange(4) == 0 else pts[rng.randrange(80)] for _ in range(k)])
    # window_reduce_kernel: a group whose chunks are all empty
    assert all(not sc.parts[b] for b in range(B, 2 * B))
    sc.seen.add("window_reduce_kernel: a group whose chunks are all empty")


def _script(m, pts, G_chunk):
    """One chunk's bucket sums, written from the top bucket down against the running sums.  Per cycle of eight buckets: a point
    (both sums copy it), an empty bucket (`tot += run` adds a record to itself: a doubling), the running sum itself (`run` doubles),
    its negative (`run` cancels), a point (`run` restarts), -(tot + run) (`tot` cancels), a point (`tot` restarts), an empty bucket."""
    G = m.G
    sums, run, tot = [], None, None
    for i in range(G_chunk):
        step = i % 8
        if step in (0, 4, 6):
            S = pts.pop()
        elif step in (1, 7):
            S = None
        elif step == 2:
            S = run
        elif step == 3:
            S = G.neg(run)
        else:
            S = G.neg(G.add(tot, run))
        run = G.add(run, S)
        tot = G.add(tot, run)
        sums.append(S)
    return sums[::-1]   # ascending bucket order


def _chains(sc, rng):
    """every chunk of buckets is a script for bucket_reduce_kernel's two running sums; chunks with equal and with opposite sums for
    window_reduce_kernel's tree where a group has more than one chunk"""
    m, G = sc.m, sc.m.G
    Gc = sc.chunk
    cpw = B // Gc
    pts = list(m.pts)
    rng.shuffle(pts)
    chunks = []   # per group, per chunk: ascending bucket sums
    for w in range(GROUPS):
        row = [_script(m, pts, Gc) for _ in range(cpw)]
        if cpw == 4:
            if w == 0:
                row[2] = list(row[0])                              # tree: task 0 += task 2 doubles
                row[3] = [G.neg(S) for S in row[1]]                # tree: task 1 += task 3 cancels
        elif cpw == 2:
            row[1] = list(row[0]) if w == 0 else [G.neg(S) for S in row[0]]
        chunks.append(row)
    for w in range(GROUPS):
        for ch in range(cpw):
            run, tot, rt, tt = m.chunk(chunks[w][ch])
            # the first cycle of eight, from the top bucket down
            assert rt[:7] == ["copy", "skip", "dbl", "cancel", "copy", "hot", "hot"], rt
            assert tt[:7] == ["copy", "dbl", "dbl", "skip", "hot", "cancel", "copy"], tt
            for b, S in enumerate(chunks[w][ch]):
                if S is not None:   # one partial sum, or two that add up to S (bucket_combine_kernel runs too)
                    if rng.randrange(3) == 0:
                        X = pts[rng.randrange(len(pts))]
                        rest = G.add(S, G.neg(X))
                        sc.put(w * B + ch * Gc + b, [X, rest] if rest is not None else [S])
                    else:
                        sc.put(w * B + ch * Gc + b, [S])
        # window_reduce_kernel's tree over the chunks' plain sums (plane 1) and weighted sums (plane 0)
        for k in (0, 1):
            _, tags = m.tree([m.chunk(c)[k] for c in chunks[w]], WIN_TASKS[m.g2])
            hits = [t for t in tags if t in ("dbl", "cancel")]
            if cpw == 4:
                assert hits == (["dbl", "cancel"] if w == 0 else []), (w, k, hits)
            elif cpw == 2:
                assert hits == (["dbl"] if w == 0 else ["cancel"]), (w, k, hits)
            else:
                assert hits == []
    sc.seen.update(["bucket_reduce_kernel: run doubles (equal sums in adjacent buckets)", "bucket_reduce_kernel: tot += run adds a record to itself",
                    "bucket_reduce_kernel: run cancels and restarts", "bucket_reduce_kernel: tot cancels and restarts"])
    if cpw > 1:
        sc.seen.update(["window_reduce_kernel: chunks with equal sums", "window_reduce_kernel: chunks with opposite sums"])


def heavy_buckets(sc):
    return [b for b, n in enumerate(sc.nparts) if n > HEAVY_PARTS]


def _next_nonempty(nparts, b):
    for k in range(b + 1, len(nparts)):
        if nparts[k]:
            return k
    return None


def wrong_list_shows(sc, b):
    """What the heavy stage does to scenario `sc` when it is told, from another job's heavy list, that bucket b is heavy:
    "overwrite": b is empty, so the identity goes into the slot at its offset -- the first slot of the next bucket that holds anything --
    and that bucket holds ONE record, not the identity, which is lost ("overwrite, adjacent": it is bucket b + 1);
    "twice": b holds 2 .. HEAVY_PARTS records, the stage sums them into the first slot and bucket_combine_kernel adds all but the first
    a second time, and those do not sum to the identity.  None: neither (the bucket sum survives)."""
    n = sc.nparts[b]
    if n == 0:
        k = _next_nonempty(sc.nparts, b)
        if k is not None and sc.nparts[k] == 1 and sc.sums[k] is not None:
            return "overwrite, adjacent" if k == b + 1 else "overwrite"
    elif 2 <= n <= HEAVY_PARTS:
        tail = None
        for P, _, _ in sc.parts[b][1:]:
            tail = sc.m.G.add(tail, P)
        if tail is not None:
            return "twice"
    return None


def _complement(sc, rng):
    """Heavy buckets where "combine" has light or empty ones, bucket 0 and the last bucket among them; one of combine's heavy buckets is
    empty here with exactly one record in the bucket after it (a heavy stage run from combine's list would write the identity over that
    record), the other holds three records (combined a second time, the sum changes).  Two more heavy buckets sit where a heavy stage
    run from THIS scenario's list shows in "combine" and in "chains" (wrong_list_shows), for the batches with this scenario at index 0."""
    m = sc.m
    pts = list(m.pts)
    rng.shuffle(pts)
    M = GROUPS * B
    other = {name: scenario(m.curve, m.g2, sc.merged, sc.chunk, name) for name in SCENARIOS}
    Hc = heavy_buckets(other["combine"])
    assert len(Hc) >= 2 and 0 not in Hc and M - 1 not in Hc, Hc
    hb_one, hb_mid = max(Hc), min(Hc)
    assert hb_one + 1 not in Hc and hb_one + 1 < M - 1
    taken = set(Hc) | {hb_one + 1}
    heavy = {0, M - 1}
    for name in SCENARIOS:
        o = other[name]
        cand = [b for b in range(1, M - 1) if b not in taken and wrong_list_shows(o, b)]
        assert cand, "no bucket of %s on which a foreign heavy list would show" % name
        best = [b for b in cand if wrong_list_shows(o, b).startswith("overwrite")] or cand
        heavy.add(best[0])
    assert not heavy & taken
    for k, b in enumerate(sorted(heavy)):
        n = HEAVY_PARTS + 1 + 5 * k
        sc.put(b, [None if i % 7 == 3 else pts[(i * 5 + 11 * k) % 90] for i in range(n)], "heavy here, not in combine (%d partial sums)" % n)
    sc.put(hb_one + 1, [pts[91]], "one record behind a bucket that is heavy in combine and empty here")
    sc.put(hb_mid, [Rep(pts[92], 6, 0), Rep(pts[93], 0, 3), Rep(pts[94], 3, 2)], "three records where combine is heavy")
    light = []
    for b in range(M):
        if b in heavy or b in (hb_one, hb_one + 1, hb_mid):
            continue
        k = rng.randrange(4)
        if k:
            sc.put(b, [None if rng.randrange(5) == 0 else pts[rng.randrange(90)] for _ in range(k)])
            light.append(b)
    # neither as many buckets with records nor as many records as the scenarios it shares a batch with: random buckets go until so
    def clash():
        used, total = sum(1 for q in sc.parts if q), sum(len(q) for q in sc.parts)
        return any(used == sum(1 for n in o.nparts if n) or total == sum(o.nparts) for o in other.values()) or total in (0, 1)
    while clash():
        sc.parts[light.pop()] = []
    assert not sc.parts[hb_one] and len(sc.parts[hb_one + 1]) == 1


def _empty(sc, rng):
    """no records at all"""


def _single(sc, rng):
    """one record in one bucket"""
    sc.put(rng.randrange(1, GROUPS * B - 1), [sc.m.pts[rng.randrange(len(sc.m.pts))]], "the only record")


def batch_conditions(curve, merged, chunk, batch):
    """What makes a wrong per-job pointer show, asserted with the model alone for every job at an index >= 1 of a batch:
      heavy     a bucket that is heavy in it and not at index 0: reading index 0's heavy list leaves that bucket uncombined
      shows     a bucket that is heavy at index 0 and on which index 0's heavy list changes this job's sums (wrong_list_shows): empty
                here in front of a lone record, or 2 .. HEAVY_PARTS records that get combined twice.  "complement" behind "combine"
                has both, the lone record in the very next bucket
      offsets   another number of buckets with records, another record count and other slot offsets than index 0
    The conditions are about the cases, not about a run.  Where one cannot hold it is not asked for: a second copy of index 0 has the same
    offsets and lists by construction (that batch is about the buffers); "empty" and "single" have no heavy bucket and nothing, or one
    record, to spoil -- their offsets still differ; "chains" stays as it was, so it has no heavy bucket of its own and `shows` holds for
    it only where combine's heavy buckets happen to fall well (reported, not asked for); and `shows` needs a heavy bucket at index 0.
    Every batch of different scenarios has `heavy` at some index, and `shows` at some index if index 0 has a heavy bucket.
    Returns {index: the conditions that hold} after asserting every one that can."""
    scs = [scenario(curve, False, merged, chunk, name) for name in batch]
    first = scs[0]
    H0 = set(heavy_buckets(first))
    off0 = slot_offsets(first.nparts)
    held = {}
    for y in range(1, len(batch)):
        sc, name = scs[y], batch[y]
        got = set()
        if name == batch[0]:
            assert sc.nparts == first.nparts
            held[y] = got
            continue
        if set(heavy_buckets(sc)) - H0:
            got.add("heavy")
        got |= {wrong_list_shows(sc, b) for b in H0 if sc.nparts[b] <= HEAVY_PARTS} - {None}
        if got & {"overwrite", "overwrite, adjacent", "twice"}:
            got.add("shows")
        if (sum(1 for n in sc.nparts if n) != sum(1 for n in first.nparts if n) and sum(sc.nparts) != sum(first.nparts)
                and slot_offsets(sc.nparts) != off0):
            got.add("offsets")
        want = {"offsets"}
        if name in ("combine", "complement"):
            want.add("heavy")
        if H0 and name in ("combine", "complement"):
            want.add("shows")
        if batch[0] == "combine" and name == "complement":
            want |= {"overwrite, adjacent", "twice"}
        assert want <= got, (batch, y, name, want - got)
        held[y] = got
    if len(set(batch)) > 1:
        assert any("heavy" in v for v in held.values()), batch
        assert not H0 or any("shows" in v for v in held.values()), batch
    return held


def slot_offsets(nparts):
    out, total = [], 0
    for n in nparts:
        out.append(total)
        total += n
    return out + [total]


@functools.lru_cache(maxsize=None)
def model(curve, g2):
    return Model(curve, g2)


@functools.lru_cache(maxsize=None)
def scenario(curve, g2, merged, chunk, name):
    sc = Scenario(model(curve, g2), merged, chunk, name)
    rng = random.Random("reduce/%s/%d/%d/%d/%s" % (curve, g2, merged, chunk, name))
    {"combine": _combine, "chains": _chains, "complement": _complement, "empty": _empty, "single": _single}[name](sc, rng)
    return sc.finish(rng)


def configs():
    return [(curve, g2, merged, chunk) for curve in ("bls12_381", "bn254") for g2 in (False, True) for merged in (False, True)
            for chunk in CHUNKS]


def batch_configs():
    """the batch lab is G1 only: the prover batches no G2 reductions"""
    return [cfg for cfg in configs() if not cfg[1]]


def batch_modes(batch):
    """None: together; a tuple: the early subset"""
    return (None,) + (EARLY_SUBSETS.get(len(batch), ()) if len(set(batch)) > 1 else ())


def config_id(curve, g2, merged, chunk):
    return "%s-%s-%s-G%d" % (curve, "g2" if g2 else "g1", "merged" if merged else "per_window", chunk)


def combine_case_names():
    """the named buckets of the "combine" scenario (the same list for every configuration)"""
    return sorted(scenario(*configs()[0], "combine").named.values())
