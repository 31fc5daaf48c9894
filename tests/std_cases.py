"""Shared cases and models of the standard-form lab, g16_host_std_op / g16_dev_std_op (TEST INFRASTRUCTURE, no GPU): single operations
of csrc/field.hpp (Fp<P>, Fp2<P>) and csrc/curve.hpp (Affine<F>, XYZZ<F>) on the ABI's own words.

Field values are handled as STORED residues (what the 32-bit words hold, below p); the expected results are plain integers mod p:
a + b, a - b, a b R^-1 (the Montgomery product), a R^-1 (to_canonical), a R (from_canonical); an inverse is checked as
a * got * R^-1 = R, that is plain(a) * plain(got) = 1.  For the product there is a second model, cios32: a limb-level restatement of
Fp::mul_cios32 that returns the value before reduce_once and, per row, m, c1 + c2 and the running value.  With it the generator FINDS
the operand pairs the issue names (value before the reduction in [p, 2 p) and below p, a row whose m is 0, the pairs that maximise
c1 + c2) and asserts on every row of every product case that c1 + c2 < 2^32 and the running value < 2 p: the claim of the comment at
`t[N - 1] = c1 + c2`, for all four fields.

Group points come from table_cases.point_classes / pool (multiples of the generator, the identity, (x, 0), (0, y), the G2 order-4
point, points of other curves: the formulas never read b) and the expected values from table_cases.model, the plain affine law on
any (x, y).  A raw XYZZ record of P under the scale s is (x s^2, y s^3, s^2, s^3).
Every property a case is named after is asserted here with the models alone, before any library call."""
import functools
import random

import fp30_cases as fc
import table_cases as tb

CURVES = ("bls12_381", "bn254")
KIND = {"fr": 0, "fq": 1, "fq2": 2, "g1": 3, "g2": 4}
W32 = 0xFFFFFFFF

# form name -> (id, operand slots, output slots); the group forms count in coordinates (C slots each), mul_bits takes two more slots
FP_FORMS = {"add": (0, 2, 1), "sub": (1, 2, 1), "neg": (2, 1, 1), "dbl": (3, 1, 1), "mul": (4, 2, 1), "sqr": (5, 1, 1), "inverse": (6, 1, 1),
            "to_canonical": (7, 1, 1), "from_canonical": (8, 1, 1), "flags": (9, 2, 1), "mul32": (14, 2, 1), "sqr32": (15, 1, 1),
            "from_canonical32": (18, 1, 1)}
FP2_FORMS = {"add": (0, 4, 2), "sub": (1, 4, 2), "neg": (2, 2, 2), "dbl": (3, 2, 2), "mul": (4, 4, 2), "sqr": (5, 2, 2), "inverse": (6, 2, 2)}
GROUP_FORMS = {"add_affine": (0, 4, 4), "add": (1, 8, 4), "dbl": (2, 4, 4), "dbl_affine": (3, 2, 4), "neg": (4, 4, 4), "mul_bits": (5, 4, 4),
               "to_affine": (6, 4, 2)}
TWIN32 = {"mul": "mul32", "sqr": "sqr32", "from_canonical": "from_canonical32"}   # operator*'s forms -> mul_cios32 by name


def forms(kind):
    return FP_FORMS if kind in ("fr", "fq") else FP2_FORMS if kind == "fq2" else GROUP_FORMS


def slots(kind, form):
    """(form id, operand slots, output slots) of a kind's form"""
    fid, i, o = forms(kind)[form]
    if kind in ("g1", "g2"):
        c = 2 if kind == "g2" else 1
        i, o = i * c + (2 if form == "mul_bits" else 0), o * c
    return fid, i, o


PARAMS = [(curve, kind, form) for curve in CURVES for kind in KIND for form in forms(kind)]


class Case:
    __slots__ = ("slots", "check", "what")

    def __init__(self, slots, check, what):
        self.slots, self.check, self.what = slots, check, what


# ---- the fields --------------------------------------------------------------------------------------------------------------------
class Std:
    """a base field in the standard form: N 32-bit words, R = 2^(32 N)"""

    def __init__(self, curve, which):
        f = fc.Field(curve, which)
        self.curve, self.which, self.name, self.p = curve, which, f.name, f.p
        self.N = f.NW
        self.R = f.Rstd
        self.Rp = self.R % self.p
        self.rinv = pow(self.R, -1, self.p)
        self.INV = (-pow(self.p, -1, 1 << 32)) % (1 << 32)
        self.pw = self.words(self.p)

    def words(self, v):
        assert 0 <= v < self.R
        return [(v >> (32 * i)) & W32 for i in range(self.N)]

    def value(self, w):
        assert len(w) == self.N
        return sum(int(x) << (32 * i) for i, x in enumerate(w))

    def mont_mul(self, a, b):
        return a * b * self.rinv % self.p


@functools.lru_cache(maxsize=None)
def std(curve, which):
    return Std(curve, which)


def cios32(f, a, b):
    """Fp::mul_cios32 word by word on the stored values a, b.  Returns (the value before reduce_once, [(m, c1 + c2, running value)] per
    row); nothing is truncated that the C++ does not truncate, except that c1 + c2 is kept exact so that an overflow would show"""
    av, bv, pw, N = f.words(a), f.words(b), f.pw, f.N
    t = [0] * N
    rows = []
    for i in range(N):
        bi = bv[i]
        x = av[0] * bi + t[0]
        m = ((x & W32) * f.INV) & W32
        y = m * pw[0] + (x & W32)
        assert y & W32 == 0
        c1, c2 = x >> 32, y >> 32
        for j in range(1, N):
            x = av[j] * bi + t[j] + c1
            assert x < 1 << 64
            c1 = x >> 32
            y = m * pw[j] + (x & W32) + c2
            assert y < 1 << 64
            c2 = y >> 32
            t[j - 1] = y & W32
        t[N - 1] = c1 + c2
        rows.append((m, c1 + c2, sum(v << (32 * k) for k, v in enumerate(t))))
    return rows[-1][2], rows


def assert_rows(f, a, b):
    """the comment's claim on every row; returns (pre, rows)"""
    pre, rows = cios32(f, a, b)
    for i, (m, cc, run) in enumerate(rows):
        assert cc < 1 << 32, "%s: row %d of %x * %x: c1 + c2 = %x does not fit 32 bits" % (f.name, i, a, b, cc)
        assert run < 2 * f.p, "%s: row %d of %x * %x: running value %x is not below 2 p" % (f.name, i, a, b, run)
    want = f.mont_mul(a, b)
    assert pre in (want, want + f.p), "%s: %x * %x: the limb model disagrees with a b R^-1" % (f.name, a, b)
    return pre, rows


@functools.lru_cache(maxsize=None)
def classes(curve, which):
    """[(name, stored value)]: the operand classes of the issue, every value below p, no value twice"""
    f = std(curve, which)
    p, N = f.p, f.N
    rng = random.Random("std/classes/%s" % f.name)
    out = [("0", 0), ("1", 1), ("2", 2), ("R mod p (one)", f.Rp), ("R^2 mod p", f.R * f.R % p), ("p - 1", p - 1), ("p - 2", p - 2),
           ("(p - 1) / 2", (p - 1) // 2), ("(p + 1) / 2", (p + 1) // 2)]
    k = 0
    while (1 << k) < p:
        out += [("2^%d" % k, 1 << k), ("2^%d - 1" % k, (1 << k) - 1)]
        k += 1
    for i in range(N):
        v = W32 << (32 * i)
        if v < p:
            out.append(("word %d all ones" % i, v))
    low = (1 << (32 * (N - 1))) - 1                     # every word at 2^32 - 1 as far as that stays below p: the low words, then the top
    top = (p >> (32 * (N - 1)))
    allones = low | ((top - 1) << (32 * (N - 1)))       # the top word one below p's: below p whatever p's low words are
    assert allones < p and f.words(allones)[:-1] == [W32] * (N - 1)
    out.append(("every low word all ones, the top word p's - 1", allones))
    zlow = (p >> 32) << 32
    assert zlow < p and zlow & W32 == 0 and zlow + (1 << 32) >= p
    out.append(("the largest value below p with a zero low word", zlow))
    out += [("seeded %d" % i, rng.randrange(p)) for i in range(64)]
    seen, uniq = set(), []
    for name, v in out:
        assert 0 <= v < p, name
        if v not in seen:
            seen.add(v)
            uniq.append((name, v))
    assert {0, 1, 2, f.Rp, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, zlow, allones} <= seen
    return uniq


@functools.lru_cache(maxsize=None)
def pairs(curve, which):
    """[(what, a, b)]: every class in each position beside seeded values, the classes against each other, and the named pairs"""
    f = std(curve, which)
    p = f.p
    rng = random.Random("std/pairs/%s" % f.name)
    cl = classes(curve, which)
    out = []
    for name, v in cl:
        out.append(("%s, seeded" % name, v, rng.randrange(p)))
        out.append(("seeded, %s" % name, rng.randrange(p), v))
    named = [c for c in cl if not c[0].startswith(("2^", "seeded"))] + [c for c in cl if c[0] in ("2^31", "2^32", "2^32 - 1", "2^33 - 1")]
    for na, a in named:
        for nb, b in named:
            out.append(("%s, %s" % (na, nb), a, b))
    for d, nm in ((0, "a + b = p"), (-1, "a + b = p - 1"), (1, "a + b = p + 1")):
        for a in (1, 2, (p - 1) // 2, (p + 1) // 2, p - 1, rng.randrange(2, p), rng.randrange(2, p)):
            b = p + d - a
            if 0 <= b < p:
                assert a + b == p + d
                out.append((nm, a, b))
    for a in (0, 1, p - 2, rng.randrange(p - 1), (1 << 32) - 1, (1 << 64) - 1):
        assert a + 1 < p
        out.append(("a - b with a = b - 1", a, a + 1))
    return out


@functools.lru_cache(maxsize=None)
def product_pairs(curve, which):
    """[(what, a, b, pre)] for the product forms: pairs() plus the searched and the constructed ones; the rows of every pair asserted"""
    f = std(curve, which)
    p = f.p
    rng = random.Random("std/product/%s" % f.name)
    out = []
    for what, a, b in pairs(curve, which):
        out.append((what, a, b, assert_rows(f, a, b)[0]))
    # seeded search
    hi = lo = 0
    for _ in range(400):
        a, b = rng.randrange(p), rng.randrange(p)
        pre, _ = assert_rows(f, a, b)
        if pre >= p and hi < 16:
            hi += 1
            out.append(("searched: before the reduction in [p, 2 p)", a, b, pre))
        elif pre < p and lo < 32:
            lo += 1
            out.append(("searched: before the reduction below p", a, b, pre))
    assert hi >= 4 and lo >= 32, (f.name, hi, lo)
    # directed: b = target R a^-1, so that a b R^-1 = target; a b > target R forces the value before the reduction to target + p
    for target in list(range(1, 17)) + [rng.randrange(1, p * p // f.R - 1) for _ in range(16)]:
        a = rng.randrange(1 << (p.bit_length() - 2), p)
        b = target * f.R * pow(a, -1, p) % p
        pre, _ = assert_rows(f, a, b)
        if a * b > target * f.R:
            assert pre == target + p
        out.append(("directed: a b R^-1 = %x" % target, a, b, pre))
    for target in (p - 1, p - 2, p - rng.randrange(3, 1 << 32)):    # ... and target + p is past every reachable value: it stays below p
        a = rng.randrange(1, p)
        b = target * f.R * pow(a, -1, p) % p
        pre, _ = assert_rows(f, a, b)
        assert pre == target
        out.append(("directed: a b R^-1 = p - %x" % (p - target), a, b, pre))
    assert sum(1 for c in out if p <= c[3] < 2 * p) >= 32 and sum(1 for c in out if c[3] < p) >= 32, f.name
    # a row whose m is 0: row 0 when the low words' product has a zero low word, a later row by search
    zlow = (p >> 32) << 32
    for what, a, b in (("m = 0 in row 0: b's low word is 0", rng.randrange(p), zlow), ("m = 0 in row 0: 2^16 * 2^16 in the low words", (rng.randrange(p) >> 32 << 32) | (1 << 16), (rng.randrange(p >> 32) << 32) | (1 << 16)),
                       ("m = 0 in every row: b = 0", rng.randrange(p), 0)):
        pre, rows = assert_rows(f, a, b)
        assert rows[0][0] == 0, what
        out.append((what, a, b, pre))
    a = rng.randrange(p)                                 # row 1: choose b's word 1 so that word 0 of a0 b1 + t0 vanishes
    b0 = rng.randrange(1 << 32)
    _, rows = cios32(f, a, b0)
    t0 = rows[0][2] & W32
    a0 = a & W32
    if a0 % 2 == 0:
        a, a0 = a | 1, a0 | 1
        _, rows = cios32(f, a, b0)
        t0 = rows[0][2] & W32
    b1 = (-t0 * pow(a0, -1, 1 << 32)) & W32
    b = b0 | (b1 << 32)
    pre, rows = assert_rows(f, a, b)
    assert rows[1][0] == 0 and rows[0][0] != 0
    out.append(("m = 0 in row 1 alone", a, b, pre))
    # the pairs that maximise c1 + c2: the largest words on both sides, the seeded search's best, and all classes against the big ones
    big = [p - 1, p - 2, ((p >> 32) << 32) - 1, (p >> (32 * (f.N - 1)) << (32 * (f.N - 1))) - 1, p - (1 << 32), (p - 1) // 2 * 2]
    big = [v for v in big if 0 <= v < p]
    cand = [(a, b) for a in big for b in big] + [(rng.randrange(p), rng.randrange(p)) for _ in range(200)]
    cand += [(v, w) for _, v in classes(curve, which) for w in big[:2]] + [(w, v) for _, v in classes(curve, which) for w in big[:2]]
    cand += [(a, b) for _, a, b, _ in out]             # ... and every pair above
    scored = []
    for a, b in set(cand):
        pre, rows = assert_rows(f, a, b)
        scored.append((max(r[1] for r in rows), a, b, pre))
    scored.sort(reverse=True)
    for cc, a, b, pre in scored[:16]:
        out.append(("c1 + c2 reaches %x" % cc, a, b, pre))
    global_max = scored[0][0]
    assert global_max < 1 << 32
    MAX_C1C2[f.name] = global_max
    return out


MAX_C1C2 = {}


def _w(f, v):
    return f.words(v)


def _exact(f, want_vals, what):
    want = [f.words(v) for v in want_vals]

    def check(out):
        got = [[int(x) for x in s] for s in out]
        assert got == want, "%s: got %s want %s" % (what, [hex(f.value(s)) for s in got], [hex(v) for v in want_vals])
    return check


def _fp_cases(curve, which, form):
    f = std(curve, which)
    p = f.p
    out = []
    if form in ("mul", "mul32"):
        for what, a, b, pre in product_pairs(curve, which):
            w = "%s %s [%x * %x]" % (form, what, a, b)
            out.append(Case([_w(f, a), _w(f, b)], _exact(f, [f.mont_mul(a, b)], w), w))
        return out
    if form in ("add", "sub", "flags"):
        for what, a, b in pairs(curve, which) + ([("a == a", v, v) for _, v in classes(curve, which)[:40]] if form == "flags" else []):
            w = "%s %s [%x, %x]" % (form, what, a, b)
            if form == "flags":
                want = int(a == 0) | (int(a == f.Rp) << 32) | (int(a == b) << 64)
            else:
                want = (a + b) % p if form == "add" else (a - b) % p
            out.append(Case([_w(f, a), _w(f, b)], _exact(f, [want], w), w))
        return out
    vals = list(classes(curve, which))
    if form in ("sqr", "sqr32"):
        # squares whose value before the reduction is in [p, 2 p): a^2 R^-1 = target for a small quadratic residue target
        rng = random.Random("std/sqr/%s" % f.name)
        n = 0
        while n < 32:
            a = rng.randrange(p)
            if assert_rows(f, a, a)[0] >= p:
                vals.append(("searched: the square before the reduction in [p, 2 p)", a))
                n += 1
    for name, a in vals:
        w = "%s %s [%x]" % (form, name, a)
        if form == "neg":
            chk = _exact(f, [(-a) % p], w)
        elif form == "dbl":
            chk = _exact(f, [2 * a % p], w)
        elif form in ("sqr", "sqr32"):
            assert_rows(f, a, a)
            chk = _exact(f, [f.mont_mul(a, a)], w)
        elif form == "to_canonical":
            chk = _exact(f, [a * f.rinv % p], w)
        elif form in ("from_canonical", "from_canonical32"):
            assert_rows(f, a, f.R * f.R % p)
            chk = _exact(f, [a * f.R % p], w)
        elif form == "inverse":
            def chk(o, a=a, w=w):
                got = f.value([int(x) for x in o[0]])
                assert got < p, "%s: %x is not canonical" % (w, got)
                assert f.mont_mul(a, got) == (f.Rp if a else 0) and (a or got == 0), "%s: a * %x is not one" % (w, got)
        else:
            raise KeyError(form)
        out.append(Case([_w(f, a)], chk, w))
    if form == "neg":
        assert vals[0][1] == 0
    if form == "dbl":
        assert {(p - 1) // 2, (p + 1) // 2} <= {v for _, v in vals}
    return out


# ---- Fq2 ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fq2_elements(curve):
    f = std(curve, "fq")
    p = f.p
    rng = random.Random("std/fq2/%s" % curve)
    cl = [v for n, v in classes(curve, "fq") if not n.startswith(("2^", "seeded"))] + [1 << 31, (1 << 32) - 1, 1 << 32, 1 << (p.bit_length() - 1)]
    r = lambda: rng.randrange(1, p)   # noqa: E731
    out = [("every component p - 1", (p - 1, p - 1)), ("zero", (0, 0)), ("one", (f.Rp, 0)), ("u", (0, f.Rp))]
    for v in cl:
        out += [("c0 = %x beside a seeded c1" % v, (v, r())), ("c1 = %x beside a seeded c0" % v, (r(), v)), ("both components %x" % v, (v, v))]
    for _ in range(8):
        a = r()
        out += [("c0 = 0", (0, r())), ("c1 = 0", (r(), 0)), ("c0 = c1", (a, a)), ("c0 = -c1", (a, p - a))]
    out += [("seeded", (rng.randrange(p), rng.randrange(p))) for _ in range(64)]
    return out


def _fp2_cases(curve, form):
    f = std(curve, "fq")
    p, ri = f.p, f.rinv
    els = fq2_elements(curve)
    rng = random.Random("std/fq2/%s/%s" % (curve, form))
    out = []
    if form in ("add", "sub", "mul"):
        prs = [(na + " | " + nb, a, b) for (na, a), (nb, b) in zip(els, els[7:] + els[:7])]
        prs += [(na + " | seeded", a, (rng.randrange(p), rng.randrange(p))) for na, a in els]
        prs += [("seeded | " + na, (rng.randrange(p), rng.randrange(p)), a) for na, a in els]
        prs += [(na + " | itself", a, a) for na, a in els[:40]]
        for d in (0, -1, 1):                  # component sums p, p - 1, p + 1
            a = (rng.randrange(2, p), rng.randrange(2, p))
            prs.append(("component sums p %+d" % d, a, (p + d - a[0], p + d - a[1])))
        for what, a, b in prs:
            w = "fq2 %s %s" % (form, what)
            if form == "add":
                want = [(a[0] + b[0]) % p, (a[1] + b[1]) % p]
            elif form == "sub":
                want = [(a[0] - b[0]) % p, (a[1] - b[1]) % p]
            else:
                want = [(a[0] * b[0] - a[1] * b[1]) * ri % p, (a[0] * b[1] + a[1] * b[0]) * ri % p]
            out.append(Case([_w(f, a[0]), _w(f, a[1]), _w(f, b[0]), _w(f, b[1])], _exact(f, want, w), w))
        return out
    for what, a in els + [("seeded more", (rng.randrange(p), rng.randrange(p))) for _ in range(100)]:
        w = "fq2 %s %s [%x, %x]" % (form, what, a[0], a[1])
        if form == "neg":
            chk = _exact(f, [(-a[0]) % p, (-a[1]) % p], w)
        elif form == "dbl":
            chk = _exact(f, [2 * a[0] % p, 2 * a[1] % p], w)
        elif form == "sqr":
            chk = _exact(f, [(a[0] * a[0] - a[1] * a[1]) * ri % p, 2 * a[0] * a[1] * ri % p], w)
        elif form == "inverse":
            def chk(o, a=a, w=w):
                g = [f.value([int(x) for x in s]) for s in o]
                assert g[0] < p and g[1] < p, "%s: not canonical" % w
                if a == (0, 0):
                    assert g == [0, 0], "%s: the inverse of zero is %s" % (w, g)
                else:
                    assert [(a[0] * g[0] - a[1] * g[1]) * ri % p, (a[0] * g[1] + a[1] * g[0]) * ri % p] == [f.Rp, 0], "%s: a * got is not one" % w
        else:
            raise KeyError(form)
        out.append(Case([_w(f, a[0]), _w(f, a[1])], chk, w))
    names = {n for n, _ in els}
    assert {"every component p - 1", "c0 = 0", "c1 = 0", "c0 = c1", "c0 = -c1"} <= names
    return out


# ---- the groups --------------------------------------------------------------------------------------------------------------------
class GroupCtx:
    def __init__(self, curve, g2):
        self.curve, self.g2 = curve, bool(g2)
        self.m = m = tb.model(curve, g2)
        self.f = std(curve, "fq")
        self.F, self.C, self.p = m.F, m.C, m.p
        self.r = m.cp.r
        self.cls = dict(tb.point_classes(curve, g2))
        self.pool = tb.pool(curve, g2)
        self._mul = {}

    def enc(self, e):
        """slots of a field element: the Montgomery words of its components"""
        return [self.f.words(c * self.f.Rp % self.p) for c in self.m.comps(e)]

    def dec(self, rows):
        v = [self.f.value([int(x) for x in s]) for s in rows]
        assert all(x < self.p for x in v), "a coordinate is not canonical: %s" % [hex(x) for x in v]
        return self.m.elem([x * self.f.rinv for x in v])

    def aff(self, P):
        return (self.enc(self.F.zero) * 2) if P is None else self.enc(P[0]) + self.enc(P[1])

    def raw(self, P, s):
        """the record of P under the scale s: (x s^2, y s^3, s^2, s^3)"""
        F = self.F
        assert P is not None and not F.is_zero(s)
        s2 = F.sqr(s)
        s3 = F.mul(s2, s)
        return self.enc(F.mul(P[0], s2)) + self.enc(F.mul(P[1], s3)) + self.enc(s2) + self.enc(s3)

    def raw_any(self, rec):
        """(x, y, zz, zzz) as given: the identity's forms"""
        return [s for e in rec for s in self.enc(e)]

    def point_of(self, rows, what):
        """the affine point of a raw record the library returned, with zz^3 = zzz^2 checked; None when zz = 0"""
        F, C = self.F, self.C
        x, y, zz, zzz = (self.dec(rows[i * C:(i + 1) * C]) for i in range(4))
        if F.is_zero(zz):
            return None
        assert F.mul(F.sqr(zz), zz) == F.sqr(zzz), "%s: zz^3 != zzz^2" % what
        return (F.mul(x, self.m.inv(zz)), F.mul(y, self.m.inv(zzz)))

    def mul(self, P, k):
        """k P by the model's plain double-and-add; nothing is reduced modulo a group order"""
        key = (P, k)
        if key not in self._mul:
            acc = None
            for i in range(k.bit_length() - 1, -1, -1):
                acc = self.m.dbl(acc)
                if (k >> i) & 1:
                    acc = self.m.add(acc, P)
            self._mul[key] = acc
        return self._mul[key]


@functools.lru_cache(maxsize=None)
def gctx(curve, g2):
    return GroupCtx(curve, bool(g2))


def _raw_check(g, want, what):
    def check(o):
        got = g.point_of(o, what)
        assert got == want, "%s: got %s want %s" % (what, got, want)
    return check


def _group_cases(curve, kind, form):
    g = gctx(curve, kind == "g2")
    m, F, p, C, f = g.m, g.F, g.p, g.C, g.f
    rng = random.Random("std/group/%s/%s/%s" % (curve, kind, form))
    rnd = lambda: m.elem([rng.randrange(1, p) for _ in range(C)])   # noqa: E731
    mult = g.cls["multiple of the generator"]
    pts = g.pool
    stale = (rnd(), rnd(), F.zero, rnd())
    ident_forms = [("identity: all zero", g.raw_any((F.zero,) * 4)), ("identity: zz = 0, stale x y zzz", g.raw_any(stale))]
    out = []

    def records(P, tag):
        """[(what, slots)] of P as a raw record: scale 1, a random scale; the identity in its forms"""
        if P is None:
            return list(ident_forms)
        return [("%s, scale 1" % tag, g.raw(P, F.one)), ("%s, seeded scale" % tag, g.raw(P, rnd()))]

    def tag_of(P):
        for name, ps in g.cls.items():
            if P in ps:
                return name
        return "point"

    if form in ("add_affine", "add"):
        prs = []   # (what, P, Q, kind the generator asserts)
        for i in range(6):
            P, Q = mult[i], mult[(i + 3) % 12]
            prs += [("P + Q", P, Q, "ADD"), ("P + P", P, P, "DBL"), ("P + (-P)", P, m.neg(P), "ZERO"), ("P + O", P, None, "TAKE_P"), ("O + Q", None, Q, "TAKE_Q")]
        prs.append(("O + O", None, None, "ZERO"))
        for P in g.cls["(x, 0)"]:
            prs += [("(x, 0) + (x, 0)", P, P, "ZERO"), ("(x, 0) + Q", P, mult[2], "ADD"), ("Q + (x, 0)", mult[2], P, "ADD")]
        for P in g.cls["(0, y)"]:
            D = m.dbl(P)
            assert D == m.neg(P)
            prs += [("(0, y) + (0, y)", P, P, "DBL"), ("(0, y) + 2 (0, y)", P, D, "ZERO"), ("2 (0, y) + (0, y)", D, P, "ZERO"), ("Q + (0, y)", mult[1], P, "ADD")]
        if g.g2:
            for name in ("y = (y0, 0)", "y = (0, y1)", "x = (x0, 0), y = 0", "x = (0, x1), y = 0", "order 4"):
                for P in g.cls[name]:
                    prs += [("%s: P + P" % name, P, P, "ZERO" if F.is_zero(P[1]) else "DBL"), ("%s: P + (-P)" % name, P, m.neg(P), "ZERO"),
                            ("%s: P + Q" % name, P, mult[5], "ADD"), ("%s: Q + P" % name, mult[5], P, "ADD")]
            Q4 = g.cls["order 4"][0]
            prs.append(("order 4: Q + 2 Q", Q4, m.dbl(Q4), "ADD"))
        for n in range(40):
            P, Q = pts[rng.randrange(len(pts))], pts[rng.randrange(len(pts))]
            if P is not None and Q is not None and P[0] == Q[0] and Q not in (P, m.neg(P)):
                continue   # two points of DIFFERENT curves over one x: no curve holds both, no law applies
            prs.append(("pool pair %d" % n, P, Q, m.kind(P, Q)))
        seen = set()
        for what, P, Q, k in prs:
            assert m.kind(P, Q) == k, (what, m.kind(P, Q))
            seen.add(k)
            want = m.add(P, Q)
            if form == "add_affine":
                w = "%s add_affine %s" % (kind, what)
                out.append(Case(g.aff(P) + g.aff(Q), _raw_check(g, want, w), w))
            else:
                for wa, ra in records(P, "lhs"):          # scale 1 and seeded on each side: equal and different scales
                    for wb, rb in records(Q, "rhs"):
                        w = "%s add %s (%s | %s)" % (kind, what, wa, wb)
                        out.append(Case(ra + rb, _raw_check(g, want, w), w))
                if P is not None and P == Q:                # the same record on both sides: equal under EQUAL scales
                    rec = g.raw(P, rnd())
                    w = "%s add %s (one record twice)" % (kind, what)
                    out.append(Case(rec + rec, _raw_check(g, want, w), w))
        assert seen == {"ADD", "DBL", "ZERO", "TAKE_P", "TAKE_Q"}
        if form == "add":
            assert any("P + P (lhs, scale 1 | rhs, seeded scale)" in c.what for c in out) and any("P + (-P) (lhs, seeded scale | rhs, seeded scale)" in c.what for c in out)
        return out
    if form == "mul_bits":
        r = g.r
        P = mult[0]
        assert g.mul(P, r - 1) == m.neg(P) and g.mul(P, r) is None and g.mul(P, r + 1) == P     # through -P, the identity, P
        ks = [(k, 256, n) for k, n in ((0, "0"), (1, "1"), (2, "2"), (r - 1, "r - 1"), (r, "r"), (r + 1, "r + 1"), (1 << 255, "2^255"))]
        ones = (1 << 256) - 1
        ks += [(ones, nb, "all ones, %d bits" % nb) for nb in (1, 8, 255, 256)] + [(ones, 0, "all ones, 0 bits")]
        ks += [((5 << 250) | 0xB5, 8, "bits set above the count 8"), ((1 << 200) | 3, 200, "bit 200 set, count 200")]
        ks += [(rng.randrange(1 << 256), 256, "seeded scalar %d" % i) for i in range(12)] + [(rng.randrange(1 << 64), 64, "seeded 64-bit scalar %d" % i) for i in range(4)]
        todo = [(P, k, nb, n, "generator") for k, nb, n in ks]
        todo += [(mult[3], r - 1, 256, "r - 1", "4 G"), (mult[3], r + 1, 256, "r + 1", "4 G"), (None, 12345, 256, "12345", "identity")]
        small = list(g.cls["(x, 0)"][:1]) + list(g.cls["(0, y)"])
        if g.g2:
            small += g.cls["order 4"] + g.cls["y = (y0, 0)"] + g.cls["y = (0, y1)"] + g.cls["x = (x0, 0), y = 0"]
        for Q in small:                                    # small orders: the running sum meets +-Q
            for k, nb, n in ((1, 256, "1"), (2, 256, "2"), (3, 256, "3"), (4, 8, "4"), (5, 8, "5"), (7, 3, "7"), (0xB6, 8, "0xb6"), (rng.randrange(1 << 32), 32, "seeded 32 bits")):
                todo.append((Q, k, nb, n, tag_of(Q)))
        for Q in g.cls["(0, y)"]:
            assert g.mul(Q, 3) is None and g.mul(Q, 4) == Q
        for i, (Q, k, nb, n, tag) in enumerate(todo):
            want = g.mul(Q, k & ((1 << nb) - 1)) if Q is not None else None
            recs = records(Q, tag)
            what, rec = recs[i % len(recs)]
            w = "%s mul_bits k = %s, %d bits, %s" % (kind, n, nb, what)
            kw = [(k >> (32 * j)) & W32 for j in range(8)] + [0] * (f.N - 8)
            out.append(Case(rec + [kw, [nb] + [0] * (f.N - 1)], _raw_check(g, want, w), w))
        return out
    # unary forms over every point of the pool
    for P in pts + [m.dbl(Q) for Q in pts if Q is not None and m.dbl(Q) is not None][:12]:
        tag = tag_of(P) if P is not None else "identity"
        if form == "dbl_affine":
            w = "%s dbl_affine %s" % (kind, tag)
            out.append(Case(g.aff(P), _raw_check(g, m.dbl(P), w), w))
            continue
        for what, rec in records(P, tag) + (records(P, tag) if P is not None else []):
            w = "%s %s %s" % (kind, form, what)
            if form == "dbl":
                chk = _raw_check(g, m.dbl(P), w)
            elif form == "neg":
                chk = _raw_check(g, m.neg(P), w)
            elif form == "to_affine":
                def chk(o, P=P, w=w):
                    got = [[int(x) for x in s] for s in o]
                    assert got == g.aff(P), "%s: got %s want %s" % (w, got, g.aff(P))
            else:
                raise KeyError(form)
            out.append(Case(rec, chk, w))
    if form in ("dbl", "dbl_affine"):
        for P in g.cls["(x, 0)"]:
            assert m.dbl(P) is None
        if g.g2:   # y.dbl() has one zero component and must not read as zero
            for name in ("y = (y0, 0)", "y = (0, y1)"):
                P = g.cls[name][0]
                d = F.add(P[1], P[1])
                assert (d[0] == 0) != (d[1] == 0) and m.dbl(P) is not None
    return out


@functools.lru_cache(maxsize=None)
def _cases(curve, kind, form):
    if kind in ("fr", "fq"):
        out = _fp_cases(curve, kind, form)
        assert len(out) >= 256, (curve, kind, form, len(out))
    elif kind == "fq2":
        out = _fp2_cases(curve, form)
        assert len(out) >= 256, (curve, kind, form, len(out))
    else:
        out = _group_cases(curve, kind, form)
        assert len(out) >= 24, (curve, kind, form, len(out))
    fid, nin, nout = slots(kind, form)
    N = std(curve, "fr" if kind == "fr" else "fq").N
    assert all(len(c.slots) == nin and all(len(s) == N for s in c.slots) for c in out), (curve, kind, form)
    return out


def cases(curve, kind, form):
    return list(_cases(curve, kind, form))


def words_per_slot(curve, kind):
    return std(curve, "fr" if kind == "fr" else "fq").N


def operands(curve, kind, form, n=None):
    """(cases cycled to n tuples, the operand array)"""
    import numpy as np

    cs = cases(curve, kind, form)
    if n is not None:
        cs = [cs[i % len(cs)] for i in range(n)]
    return cs, np.ascontiguousarray(np.array([c.slots for c in cs], dtype=np.uint32))


def check_all(cs, out):
    for i, (c, o) in enumerate(zip(cs, out)):
        try:
            c.check(o)
        except AssertionError as e:
            raise AssertionError("tuple %d (%s): %s" % (i, c.what, e)) from None


def run_host(curve, kind, form, ops):
    """g16_host_std_op on an operand array; the output array, prefilled so that an unwritten word shows"""
    import ctypes as C

    import numpy as np

    import groth16_amd

    lib = groth16_amd.lib()
    fid, nin, nout = slots(kind, form)
    N = words_per_slot(curve, kind)
    assert ops.shape[1:] == (nin, N)
    out = np.full((len(ops), nout, N), 0xDEADBEEF, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = lib.c.g16_host_std_op(fc.CURVE_ID[curve], KIND[kind], fid, ops.ctypes.data_as(u32p), len(ops), out.ctypes.data_as(u32p))
    assert rc == 0, (curve, kind, form, rc)
    return out


# ---- the operand file of tests/std_lab_replay.cpp ----------------------------------------------------------------------------------
def dump_operands(path, run):
    """Write the operand tuples of every (curve, kind, form), with the outputs run(curve, kind, form, operand array) -> uint32 array
    gave, to one binary file for tests/std_lab_replay.cpp.  Little-endian uint32 records: curve id, kind, form id, n, operand slots,
    output slots, words per slot | n * nin * N operand words | n * nout * N output words.  Returns (records, tuples)."""
    import numpy as np

    records = tuples = 0
    with open(path, "wb") as fh:
        for curve, kind, form in PARAMS:
            fid, nin, nout = slots(kind, form)
            N = words_per_slot(curve, kind)
            cs, ops = operands(curve, kind, form)
            out = np.ascontiguousarray(run(curve, kind, form, ops), dtype="<u4")
            assert ops.shape == (len(cs), nin, N) and out.shape == (len(cs), nout, N)
            fh.write(np.array([fc.CURVE_ID[curve], KIND[kind], fid, len(cs), nin, nout, N], dtype="<u4").tobytes())
            fh.write(ops.astype("<u4").tobytes())
            fh.write(out.tobytes())
            records += 1
            tuples += len(cs)
    return records, tuples
