"""Cases and the big-int model for the division-step inverse, the window-table builder and one pair of the batched-affine tree
(TEST INFRASTRUCTURE, no GPU): the field-lab forms inv_plain, inv, pair_inv, jac_dbl_* and aff_pair_* (fp30_cases.lab_cases hands
them over to lab_cases() here) and the table lab, g16_dev_window_table_lab (point_classes / table_points / expected_table).

The model is a plain affine group law with a = 0 that takes ANY pair (x, y): doubling is the tangent rule (the identity when y = 0),
addition the chord rule.  Neither formula reads b, so every (x, y) is a point of SOME curve y^2 = x^3 + b' and the law is the true
one there; nothing is reduced modulo a group order (pymodel's Group.mul would do that).  That is what lets the cases leave the
prime-order subgroup, which whole proofs and MSMs on subgroup points never do:
  (x, 0)            two-torsion: Z = 2 Y Z is zero after ONE doubling -- window_table_task's `live` exit; row 0 finite, every later row
                    the identity
  (0, y)            order 3 (2 P = -P); on BLS12-381 (0, 2) lies on the curve itself
  G2  y = (y0, 0), (0, y1)       Z gets a zero COMPONENT after one doubling and must not read as the identity
  G2  x = (x0, 0) or (0, x1), y = 0     the two lanes of the pair disagree in load()'s all-zero test: the point is NOT the identity
  G2  a point Q of order 4: 2 Q = (xt, 0), so Y turns into a multiple of p that a FORMULA computed (lazy k p, not an exact zero) and
      the row after that is the identity.  With s3 = sqrt(3) in Fq2 (3 is a non-residue in both base fields, so no such point exists
      over Fq), t = 1 + s3, k = t^3 - 1:  Q = (k s^2 t, k^2 s^3) for any scale s.
Every property a case is named after is asserted here with the model alone, before any library call."""
import functools
import os
import random
import sys
from fractions import Fraction

import fp30_cases as fc

sys.path.insert(0, os.path.join(fc.ROOT, "oracle"))
import pymodel  # noqa: E402

MASK = fc.MASK
KIND = {"ADD": 0, "DBL": 1, "TAKE_P": 2, "TAKE_Q": 3, "ZERO": 4}
JAC_BOUNDS = (Fraction(29, 5), Fraction(11, 2), Fraction(3))   # window_tables.hpp: X < 5.8 p, Y < 5.5 p, Z < 3 p per component
PAIR_INV_BOUND = Fraction(3, 2)                                # batch_affine.hpp, next to pair_inverse: its callers stay below 1.5 p


class Model:
    """Fq (g2 = False) or Fq2 elements as ints / pairs, and the affine law on any (x, y); None is the identity"""

    def __init__(self, curve, g2):
        self.curve, self.g2 = curve, bool(g2)
        self.cp = pymodel.CURVES[curve]
        self.f = fc.Field(curve, "fq")
        self.p = p = self.f.p
        self.C = 2 if g2 else 1
        self.F = pymodel.Fq2(p) if g2 else pymodel.Fq1(p)
        self.gen = self.cp.g2 if g2 else self.cp.g1
        self.rinv = pow(self.f.R, -1, p)

    def comps(self, e):
        return list(e) if self.g2 else [e]

    def elem(self, c):
        return (c[0] % self.p, c[1] % self.p) if self.g2 else c[0] % self.p

    def inv(self, a):
        p = self.p
        if not self.g2:
            return pow(a, -1, p)
        ni = pow((a[0] * a[0] + a[1] * a[1]) % p, -1, p)
        return (a[0] * ni % p, -a[1] * ni % p)

    def neg(self, P):
        return None if P is None else (P[0], self.F.neg(P[1]))

    def dbl(self, P):
        F = self.F
        if P is None or F.is_zero(P[1]):
            return None
        x, y = P
        lam = F.mul(F.mul(F.from_int(3), F.sqr(x)), self.inv(F.add(y, y)))
        x3 = F.sub(F.sqr(lam), F.add(x, x))
        return (x3, F.sub(F.mul(lam, F.sub(x, x3)), y))

    def kind(self, P, Q):
        if P is None or Q is None:
            return "ZERO" if P is None and Q is None else "TAKE_Q" if P is None else "TAKE_P"
        if P[0] == Q[0]:
            return "ZERO" if self.F.is_zero(self.F.add(P[1], Q[1])) else "DBL"
        return "ADD"

    def add(self, P, Q):
        F, k = self.F, self.kind(P, Q)
        if k != "ADD":
            return {"ZERO": None, "TAKE_P": P, "TAKE_Q": Q, "DBL": self.dbl(P)}[k]
        lam = F.mul(F.sub(Q[1], P[1]), self.inv(F.sub(Q[0], P[0])))
        x3 = F.sub(F.sub(F.sqr(lam), P[0]), Q[0])
        return (x3, F.sub(F.mul(lam, F.sub(P[0], x3)), P[1]))

    @functools.lru_cache(maxsize=None)
    def chain(self, P, k):
        """2^k P"""
        return P if k == 0 else self.dbl(self.chain(P, k - 1))

    def mont(self, e):
        """canonical Montgomery residues (R' radix) of an element's components"""
        return [c * self.f.R % self.p for c in self.comps(e)]

    def plain(self, vals):
        """the element whose components are the lazy Montgomery values `vals`"""
        return self.elem([v * self.rinv for v in vals])


@functools.lru_cache(maxsize=None)
def model(curve, g2):
    return Model(curve, bool(g2))


# ---- the points ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_classes(curve, g2):
    """[(class name, [points])]: every special point with the property it is named after asserted by the model"""
    m = model(curve, g2)
    F, p = m.F, m.p
    rng = random.Random("table/points/%s/%d" % (curve, g2))
    rnd = (lambda: (rng.randrange(1, p), rng.randrange(1, p))) if g2 else (lambda: rng.randrange(1, p))
    mult = [m.gen]
    for _ in range(11):
        mult.append(m.add(mult[-1], m.gen))
    G = pymodel.groups(m.cp)[1 if g2 else 0]
    assert all(G.on_curve(P) for P in mult) and mult[1] == G.add(m.gen, m.gen) and mult[4] == G.mul(m.gen, 5)
    out = [("multiple of the generator", mult), ("identity", [None])]
    two = [(rnd(), F.zero) for _ in range(2)]
    for P in two:
        assert m.dbl(P) is None
    out.append(("(x, 0)", two))
    three = [(F.zero, rnd())]
    if curve == "bls12_381" and not g2:
        three.append((0, 2))
        assert G.on_curve((0, 2))
    for P in three:
        assert m.dbl(P) == m.neg(P) and m.add(m.dbl(P), P) is None
    out.append(("(0, y)", three))
    if g2:
        for name, y in (("y = (y0, 0)", (rng.randrange(1, p), 0)), ("y = (0, y1)", (0, rng.randrange(1, p)))):
            P = (rnd(), y)
            D = m.dbl(P)
            assert D is not None and (F.add(y, y)[0] == 0) != (F.add(y, y)[1] == 0)   # Z = 2 Y Z: one zero component, a finite point
            out.append((name, [P]))
        for name, x in (("x = (x0, 0), y = 0", (rng.randrange(1, p), 0)), ("x = (0, x1), y = 0", (0, rng.randrange(1, p)))):
            P = (x, F.zero)
            assert m.dbl(P) is None and (x[0] == 0) != (x[1] == 0)
            out.append((name, [P]))
        s3 = (0, pow(-3 % p, (p + 1) // 4, p))
        assert F.sqr(s3) == (3, 0) and pow(3, (p - 1) // 2, p) == p - 1   # sqrt(3) lives in Fq2 only
        four = []
        for s in (F.one, rnd()):
            t = F.add(F.one, s3)
            k = F.sub(F.mul(F.sqr(t), t), F.one)
            xt = F.mul(k, F.sqr(s))
            Q = (F.mul(xt, t), F.mul(F.sqr(k), F.mul(F.sqr(s), s)))
            assert m.dbl(Q) == (xt, F.zero) and not F.is_zero(Q[1]) and m.chain(Q, 2) is None
            four.append(Q)
        out.append(("order 4", four))
    return out


def pool(curve, g2):
    """every distinct point of point_classes, classes interleaved"""
    cls = point_classes(curve, g2)
    out = []
    for i in range(max(len(pts) for _, pts in cls)):
        out += [pts[i] for _, pts in cls if i < len(pts)]
    return out


# ---- the field-lab forms ---------------------------------------------------------------------------------------------------------
def _normalised(f, limbs, what):
    assert all(x <= MASK for x in limbs[:-1]), "%s: not normalised: %s" % (what, limbs)


def inverse_operands(f):
    """operands of ModInv30::inverse_plain: any value below 2^(30 NL - 3)"""
    p, B = f.p, 1 << (30 * f.NL - 3)
    rng = random.Random("table/inverse/%s" % f.name)
    ops = [0, 1, 2, 3, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, f.R % p, B - 1, B - 2]
    ops += [((1 << 30) - 1) << (30 * i) for i in range(f.NL)]                     # one limb all ones
    ops += [(1 << f.top_shift) - 1, ((B - 1) >> f.top_shift << f.top_shift) | ((1 << f.top_shift) - 1)]   # all limbs, the top as the bound allows
    for k in range(30 * f.NL - 3):
        ops += [1 << k, (1 << k) - 1]
    ops += [rng.randrange(p) for _ in range(64)] + [rng.randrange(B) for _ in range(64)]
    ops += [k * p + d for k in range(B // p + 1) for d in (0, -1, 1)]
    seen, out = set(), []
    for v in ops:
        if 0 <= v < B and v not in seen:
            seen.add(v)
            out.append(v)
    assert {k * p for k in range(B // p + 1)} <= seen and B - 1 in seen
    return out


def _inverse_cases(f, form):
    p, L = f.p, f.limbs
    out = []
    for x in inverse_operands(f):
        want = pow(x, -1, p) if x % p else 0
        what = "%s(%x)" % (form, x)
        if form == "inv_plain":
            out.append(fc.LabCase([L(x)], fc._exact(f, L(want), what), form))
            continue

        def check(o, want=want * f.R * f.R % p, what=what):
            limbs = [int(v) for v in o[0]]
            _normalised(f, limbs, what)
            v = f.value(limbs)
            assert v % p == want, "%s: wrong residue (value %x)" % (what, v)
            assert v < f.bound(Fraction(3, 2)), "%s = %.3f p, promised < 1.5 p" % (what, v / p)
        out.append(fc.LabCase([L(x)], check, form))
    return out


def _pair_inv_cases(f, rng):
    p, L = f.p, f.limbs
    bd = f.bound(PAIR_INV_BOUND)
    r2 = f.R * f.R % p
    named = [(0, 5), (5, 0), (0, 0), (1, 0), (0, 1), (p - 1, 0), (0, p - 1), (p - 1, p - 1), (f.R % p, 0), (bd - 1, bd - 1), (bd - 1, 0), (0, bd - 1)]
    named += [(0, rng.randrange(1, p)), (rng.randrange(1, p), 0)]
    lazy = []
    for a in named + [(rng.randrange(p), rng.randrange(p)) for _ in range(8)]:   # the same residues as r + p where that stays below the bound
        for k0, k1 in ((1, 0), (0, 1), (1, 1)):
            t = (a[0] + k0 * p, a[1] + k1 * p)
            if t[0] < bd and t[1] < bd:
                lazy.append(t)
    assert (p, p) in lazy and (p, 0) in lazy and (0, p) in lazy
    ops = named + lazy + fc.tuples_from(f, [bd, bd], rng, 64)
    # beyond the callers' bound: the aff_pair forms invert a pair's own denominator, qx - px + 2 p < 3 p per component
    wide = f.bound(3)
    ops += [(wide - 1, wide - 1), (2 * p, 2 * p + 1), (2 * p + 1, 0), (0, 2 * p + 1)] + [(rng.randrange(wide), rng.randrange(2 * p, wide)) for _ in range(28)]
    out = []
    for a in ops:
        what = "pair_inv(%x, %x)" % a

        def check(o, a=a, what=what):
            v = []
            for c in range(2):
                limbs = [int(x) for x in o[c]]
                _normalised(f, limbs, "%s component %d" % (what, c))
                v.append(f.value(limbs))
                # the issue's bound is 2 p; pair_inverse's comment promises 1.5 p (a one-sweep product), so that is what is asserted
                assert v[c] < f.bound(Fraction(3, 2)), "%s: component %d = %.3f p, promised < 1.5 p" % (what, c, v[c] / p)
            if a[0] % p == 0 and a[1] % p == 0:
                assert v[0] % p == 0 and v[1] % p == 0, "%s: zero must give zero, got (%x, %x)" % (what, v[0], v[1])
            else:
                assert fc.fq2_mul(a, v, p) == (r2, 0), "%s: (c0 + c1 u) * out is not R'^2: out = (%x, %x)" % (what, v[0], v[1])
        out.append(fc.LabCase([L(a[0]), L(a[1])], check, "pair_inv"))
    return out


def _jac_cases(f, form, rng):
    g2 = form.endswith("_g2_pair")
    m = model(f.curve, g2)
    F, p, C, NL, L = m.F, f.p, m.C, f.NL, f.limbs
    bds = [f.bound(b) for b in JAC_BOUNDS for _ in range(C)]    # per component: X.. Y.. Z..
    DS = (1, 2, 20, 32)

    def case(vals, d, what):
        what = "%s %s, d = %d" % (form, what, d)
        assert len(vals) == 3 * C and all(0 <= v < b for v, b in zip(vals, bds)), what
        X, Y, Z = (m.plain(vals[i * C:(i + 1) * C]) for i in range(3))
        P = None
        if not F.is_zero(Z):
            zi = m.inv(Z)
            P = (F.mul(X, F.sqr(zi)), F.mul(Y, F.mul(F.sqr(zi), zi)))
        want = m.chain(P, d)

        def check(o, want=want, what=what):
            v = []
            for i in range(3 * C):
                limbs = [int(x) for x in o[i]]
                _normalised(f, limbs, "%s, output slot %d" % (what, i))
                v.append(f.value(limbs))
                assert v[i] < bds[i], "%s: output slot %d = %.3f p, documented bound %s p" % (what, i, v[i] / p, JAC_BOUNDS[i // C])
            X3, Y3, Z3 = (m.plain(v[i * C:(i + 1) * C]) for i in range(3))
            if want is None:
                assert F.is_zero(Z3), "%s: the model reaches the identity, Z = %s" % (what, [hex(x) for x in v[2 * C:]])
                return
            assert not F.is_zero(Z3), "%s: Z is zero, the model's point is finite" % what
            zi = m.inv(Z3)
            got = (F.mul(X3, F.sqr(zi)), F.mul(Y3, F.mul(F.sqr(zi), zi)))
            assert got == want, "%s: got %s want %s" % (what, got, want)
        return fc.LabCase([L(v) for v in vals] + [fc._flag(d)[:NL]], check, form), want

    def klass(i, name):
        bd = bds[i]
        return {"0": 0, "1": 1, "p-1": p - 1, "p": p, "p+1": p + 1, "bound-1": bd - 1, "below p": rng.randrange(p), "lazy": rng.randrange(p, bd)}[name]

    CLASSES = ("0", "1", "p-1", "p", "p+1", "bound-1", "below p", "lazy")
    rnd = lambda: [rng.randrange(b) for b in bds]   # noqa: E731
    out = []
    for d in DS:
        out.append(case([b - 1 for b in bds], d, "every component at bound - 1")[0])
        for name in CLASSES:
            out.append(case([klass(i, name) for i in range(3 * C)], d, "every component %s" % name)[0])
    n = 0
    for i in range(3 * C):
        for name in CLASSES:
            v = rnd()
            v[i] = klass(i, name)
            out.append(case(v, DS[n % 4], "%s %s beside random components" % ("XYZ"[i // C] + (str(i % C) if g2 else ""), name))[0])
            n += 1
    # the named points, affine (Z = one) and under a random scale z with lazy representatives: (x z^2, y z^3, z)
    reached = set()
    for cname, pts in point_classes(f.curve, g2):
        for P in pts:
            if P is None:
                continue
            for scaled in (False, True):
                z = m.elem([rng.randrange(1, p) for _ in range(C)]) if scaled else F.one
                coords = (F.mul(P[0], F.sqr(z)), F.mul(P[1], F.mul(F.sqr(z), z)), z)
                vals = []
                for e, b in zip(coords, JAC_BOUNDS):
                    for c in m.mont(e):
                        k = rng.randrange(int(b)) if scaled else 0
                        vals.append(c + k * p if c + k * p < f.bound(b) else c)
                for d in DS:
                    cs, want = case(vals, d, "%s%s" % (cname, ", scaled" if scaled else ""))
                    assert want == m.chain(P, d)
                    out.append(cs)
                    if want is None:
                        reached.add(cname)
    assert {"(x, 0)"} <= reached and (not g2 or {"order 4", "x = (x0, 0), y = 0", "x = (0, x1), y = 0"} <= reached)
    return out


def _aff_cases(f, form, rng):
    g2 = form.endswith("_g2_pair")
    m = model(f.curve, g2)
    F, p, C, NL, L = m.F, f.p, m.C, f.NL, f.limbs
    zero = [[0] * NL] * C

    def coords(P):
        return zero + zero if P is None else [L(c) for c in m.mont(P[0])] + [L(c) for c in m.mont(P[1])]

    def case(P, Q, kind, what):
        what = "%s %s" % (form, what)
        assert m.kind(P, Q) == kind, (what, m.kind(P, Q))
        S = m.add(P, Q)
        want = coords(S) + [([int(S is None), KIND[kind]] + [0] * NL)[:NL]]

        def check(o, want=want, what=what):
            got = [[int(x) for x in s] for s in o]
            assert got[2 * C] == want[2 * C], "%s: identity flag, kind = %s, model %s" % (what, got[2 * C][:2], want[2 * C][:2])
            assert got == want, "%s: got %s want %s" % (what, got, want)
        flags = ([int(P is None), int(Q is None)] + [0] * NL)[:NL]
        return fc.LabCase([flags] + coords(P) + coords(Q), check, form)

    cls = dict(point_classes(f.curve, g2))
    mult = cls["multiple of the generator"]
    out = []
    for i in range(6):
        P, Q = mult[i], mult[(i + 3) % 12]
        out.append(case(P, Q, "ADD", "P + Q (%d)" % i))
        out.append(case(P, P, "DBL", "P + P (%d)" % i))
        out.append(case(P, m.neg(P), "ZERO", "P + (-P): equal x, y and p - y (%d)" % i))
        out.append(case(P, None, "TAKE_P", "P + O (%d)" % i))
        out.append(case(None, Q, "TAKE_Q", "O + Q (%d)" % i))
    out.append(case(None, None, "ZERO", "O + O"))
    for P in cls["(x, 0)"]:
        out.append(case(P, P, "ZERO", "(x, 0) + (x, 0)"))
        out.append(case(P, mult[2], "ADD", "(x, 0) + Q"))
    for P in cls["(0, y)"]:
        out.append(case(P, P, "DBL", "(0, y) + (0, y)"))
        out.append(case(P, m.neg(P), "ZERO", "(0, y) - (0, y)"))
        out.append(case(mult[1], P, "ADD", "P + (0, y)"))
    if g2:
        for name in ("y = (y0, 0)", "y = (0, y1)", "x = (x0, 0), y = 0", "x = (0, x1), y = 0", "order 4"):
            for P in cls[name]:
                k = "ZERO" if F.is_zero(P[1]) else "DBL"
                out.append(case(P, P, k, "%s: P + P" % name))
                out.append(case(P, m.neg(P), "ZERO", "%s: P + (-P)" % name))
                out.append(case(P, mult[5], "ADD", "%s: P + Q" % name))
                out.append(case(mult[5], P, "ADD", "%s: Q + P" % name))
        # the lanes of the pair disagree on x: one component equal, the other not (the chord rule reads no curve constant)
        for c in range(2):
            P = mult[3]
            x = list(P[0])
            x[c] = (x[c] + 1 + rng.randrange(p - 1)) % p
            for y in (P[1], F.neg(P[1]), mult[4][1]):
                out.append(case(P, (tuple(x), y), "ADD", "x equal in component %d only" % (1 - c)))
        # ... and on y: equal x, y + y' zero in one component only would be no point of P's curve; P + (-P) with a zero y component is
        P = cls["y = (y0, 0)"][0]
        assert m.neg(P)[1][1] == 0 and m.neg(P)[1][0] == p - P[1][0]
    rpts = [None] + [m.chain(P, k) for P in mult[:6] for k in range(6)]
    for n in range(64):
        P, Q = rpts[1 + rng.randrange(len(rpts) - 1)], rpts[1 + rng.randrange(len(rpts) - 1)]
        out.append(case(P, Q, m.kind(P, Q), "random pair %d" % n))
    assert {c.what for c in out} == {form}
    return out


@functools.lru_cache(maxsize=None)
def _lab_cases(curve, form):
    f = fc.Field(curve, "fq")
    rng = random.Random("table/lab/%s/%s" % (curve, form))
    if form in ("inv_plain", "inv"):
        out = _inverse_cases(f, form)
    elif form == "pair_inv":
        out = _pair_inv_cases(f, rng)
    elif form.startswith("jac_dbl"):
        out = _jac_cases(f, form, rng)
    elif form.startswith("aff_pair"):
        out = _aff_cases(f, form, rng)
    else:
        raise KeyError(form)
    nin = fc.LAB[form][1]
    assert len(out) >= 65 and all(len(c.slots) == nin and all(len(s) == f.NL for s in c.slots) for c in out), (curve, form)
    return out


def lab_cases(f, form):
    assert f.which == "fq"
    return list(_lab_cases(f.curve, form))


# ---- the table lab ---------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 2), (3, 1), (5, 4), (8, 32), (16, 16), (20, 13))   # (c, W)
SIZES = (1, 63, 64, 65)
TABLE_THREADS = 128                                              # msm.hip: lanes per workgroup of build_window_tables_kernel


def tasks_per_wave(g2):
    return 32 if g2 else 64


def big_n(g2):
    """a point count whose tasks span three workgroups, the last one partly filled"""
    per_wg = TABLE_THREADS // (2 if g2 else 1)
    return 2 * per_wg + per_wg // 2 + 7


def table_points(curve, g2, n, layout=0):
    """n points of the pool, rotated by `layout`.  For big_n the classes are laid on the wave edges instead: class k of layout L sits
    at the first and at the last task of wave k - 5 L (five full waves), for the classes that fit; the layouts together put every
    class on both edges (edge_classes says which).  Returns (points, {task index: class name} for the edge tasks)."""
    pl = pool(curve, g2)
    pts = [pl[(i + 5 * layout) % len(pl)] for i in range(n)]
    edges = {}
    if n == big_n(g2):
        T = tasks_per_wave(g2)
        cls = point_classes(curve, g2)
        full_waves = n // T
        for w in range(full_waves):
            k = w + full_waves * layout
            if k < len(cls):
                name, cpts = cls[k]
                for t in (w * T, w * T + T - 1):
                    pts[t] = cpts[-1]
                    edges[t] = name
    return pts, edges


def layouts(curve, g2):
    """how many layouts of big_n it takes to put every class on a wave's first and last task"""
    full_waves = big_n(g2) // tasks_per_wave(g2)
    return -(-len(point_classes(curve, g2)) // full_waves)


def abi_words(m, P):
    """uint64 limbs of an affine point in the ABI's form (standard Montgomery, all-zero = the identity)"""
    f = m.f
    n64 = f.NW // 2
    if P is None:
        return [0] * (2 * m.C * n64)
    out = []
    for e in P:
        for c in m.comps(e):
            v = c * f.Rstd % f.p
            out += [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n64)]
    return out


def row_words(m, P):
    """uint64 limbs of a table row: canonical x R' and y R' in the packed form's words; the identity is all zero"""
    f = m.f
    n64 = f.NW // 2
    if P is None:
        return [0] * (2 * m.C * n64)
    out = []
    for e in P:
        for v in m.mont(e):
            out += [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n64)]
    return out


def decode_row(m, words):
    """the inverse of row_words, for messages: a point, None, or the raw words if a coordinate is not canonical"""
    f = m.f
    n64 = f.NW // 2
    vals = [sum(int(w) << (64 * i) for i, w in enumerate(words[k * n64:(k + 1) * n64])) for k in range(2 * m.C)]
    if not any(vals):
        return None
    if any(v >= f.p for v in vals):
        return "not canonical: %s" % [hex(v) for v in vals]
    return (m.plain(vals[:m.C]), m.plain(vals[m.C:]))


def expected_table(curve, g2, pts, c, W):
    """[W][n] rows as row_words; row j of point i = 2^(c j) P_i"""
    m = model(curve, g2)
    return [[row_words(m, m.chain(P, c * j)) for P in pts] for j in range(W)]


# ---- the operand file of tests/field_lab_replay.cpp --------------------------------------------------------------------------------
def dump_operands(path, run):
    """Write the operand tuples of every new form that has a host twin, with the outputs run(f, form, cases) -> uint32 array gave, to
    one binary file for tests/field_lab_replay.cpp (a stand-alone program that replays them through g16_host_fp30_op, e.g. in a
    sanitizer build).  Little-endian uint32 records: curve id, field id, form id, n, operand slots, output slots, NL | n * nin * NL
    operand words | n * nout * NL output words.  Returns (records, tuples)."""
    import numpy as np

    records = tuples = 0
    with open(path, "wb") as fh:
        for f in fc.fields():
            if f.which != "fq":
                continue
            for form in fc.TABLE_FORMS:
                if form in fc.DEVICE_ONLY:
                    continue
                fid, nin, nout = fc.LAB[form]
                cs = lab_cases(f, form)
                ops = np.ascontiguousarray(np.array([c.slots for c in cs], dtype="<u4"))
                out = np.ascontiguousarray(run(f, form, cs), dtype="<u4")
                assert ops.shape == (len(cs), nin, f.NL) and out.shape == (len(cs), nout, f.NL)
                fh.write(np.array([fc.CURVE_ID[f.curve], fc.FIELD_ID[f.which], fid, len(cs), nin, nout, f.NL], dtype="<u4").tobytes())
                fh.write(ops.tobytes())
                fh.write(out.tobytes())
                records += 1
                tuples += len(cs)
    return records, tuples
