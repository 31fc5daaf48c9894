"""Shared cases and the exact model of the tower lab, g16_host_pairing_op / g16_dev_pairing_op (TEST INFRASTRUCTURE, no GPU).

For a curve and a form of the lab (include/g16_mi355x.h lists them) this module yields operand tuples as raw limb slots and a check
of the output slots.  Everything is exact: an Fq result must be a normalised limb vector with a value BELOW 2 p -- the invariant the
next operation of a chain relies on -- whose residue is the model's; a flag must equal the model's predicate; store_gt must give the
canonical Montgomery words of the model value for every representative.

The model is pymodel's: plain integers for Fq, pymodel.Fq2, and for Fq6 / Fq12 the flat ring pymodel.Fq12 = Fq[w]/(w^12 - c6 w^6 - c0),
whose representation knows nothing of the tower (pairing_model.to_ark and from_ark below convert).  Added here: from_ark, a cheap
Frobenius (w^(q^j) once per curve and j by F.pow, then a linear map) and a cheap inverse built on it (the product of the eleven
conjugates over the norm), so that no case needs a q-th or a (q^12 - 2)-th power.

Operand classes, per Fq component of every operand: the representatives 0, 1, R' mod p (the Montgomery one), p - 1, p, p + 1 and
2 p - 1, a random value below p and a random value in [p, 2 p) -- all at 2 p - 1, all zero, each of them in each position beside random
components -- then named elements (the unit, lazy zeros, subfield elements, the sparse 014 / 034 shapes, elements with zero components
for the inverses) and 64 seeded random tuples.  The forms that need cyclotomic inputs draw them from a few model-made base elements
(products, conjugates, Frobenius images, 1), each as the canonical and as shifted representatives.  Every named property (a lazy
zero, in the subfield, in the cyclotomic subgroup, a doubling's or an addition's operands) is asserted with the model alone.

Non-invertible inputs: Q30::inverse is Fermat's (a^(p - 2)), so the inverse of a zero residue is 0, and the T2 / T6 / T12 inverses of a
zero element are zero in every component."""
import os
import random
import sys
from functools import lru_cache

import fp30_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pymodel as pm  # noqa: E402

import pairing_model as pmod  # noqa: E402

CURVES = ("bls12_381", "bn254")
MASK = fc.MASK

# name -> (form id, operand slots, output slots); a slot is NL 32-bit words
FORMS = {
    "q_add": (0, 2, 1), "q_sub": (1, 2, 1), "q_neg": (2, 1, 1), "q_dbl": (3, 1, 1), "q_mul": (4, 2, 1), "q_sqr": (5, 1, 1),
    "q_is_zero": (6, 1, 1), "q_eq": (7, 2, 1), "q_inverse": (8, 1, 1), "q_std_roundtrip": (9, 1, 1),
    "t2_add": (10, 4, 2), "t2_sub": (11, 4, 2), "t2_neg": (12, 2, 2), "t2_conj": (13, 2, 2), "t2_dbl": (14, 2, 2), "t2_scale": (15, 3, 2),
    "t2_mul": (16, 4, 2), "t2_sqr": (17, 2, 2), "t2_inverse": (18, 2, 2), "t2_mul_by_xi": (19, 2, 2), "t2_eq": (20, 4, 1),
    "t6_add": (30, 12, 6), "t6_sub": (31, 12, 6), "t6_neg": (32, 6, 6), "t6_mul": (33, 12, 6), "t6_mul_by_v": (34, 6, 6),
    "t6_inverse": (35, 6, 6),
    "t12_mul": (40, 24, 12), "t12_sqr": (41, 12, 12), "t12_cyc_sqr": (42, 12, 12), "t12_conj": (43, 12, 12), "t12_inverse": (44, 12, 12),
    "t12_is_zero": (45, 12, 1),
    "frob": (50, 13, 12), "equal": (51, 24, 1), "store_gt": (52, 12, 12), "load_store_gt": (53, 12, 12), "ell": (54, 20, 12),
    "dbl_step": (55, 6, 12), "add_step": (56, 10, 12), "frob_twist": (57, 5, 4), "cyc_pow": (58, 13, 12), "cyc_pow_bits": (59, 13, 12),
    "exp_by_x": (60, 12, 12), "final_exp": (61, 12, 13), "g1_on_curve": (62, 2, 1), "g2_on_curve": (63, 4, 1),
}
# a lane's chain is milliseconds long here: the device tier cycles these to 129 tuples, not 2049
LONG_FORMS = ("final_exp", "cyc_pow_bits")


class Case:
    """slots: one NL-word list per operand slot; check(out_slots) raises AssertionError with a message"""
    __slots__ = ("slots", "check", "what")

    def __init__(self, slots, check, what):
        self.slots, self.check, self.what = slots, check, what


class Ctx:
    def __init__(self, curve):
        self.curve = curve
        self.f = f = fc.Field(curve, "fq")
        self.cp = pm.CURVES[curve]
        self.p, self.NL, self.R = f.p, f.NL, f.R
        self.Rinv = pow(f.R, -1, f.p)
        self.one = f.R % f.p                 # the Montgomery one
        self.F = pm.Fq12(self.cp)
        self.F2 = pm.Fq2(self.cp.q)
        self.s = pm._TOWER[curve]["s"]       # xi = s + u
        self.m_twist = pm._TOWER[curve]["twist"] == "M"
        self.x = pmod.LOOP[curve]["x"]

    def raw(self, res, k=0):
        """the representative res R' mod p + k p"""
        return res * self.R % self.p + k * self.p

    def res(self, raw):
        return raw * self.Rinv % self.p

    def flag(self, v):
        return [int(v)] + [0] * (self.NL - 1)


@lru_cache(maxsize=None)
def ctx(curve):
    return Ctx(curve)


# ---- the model helpers added to pairing_model's ------------------------------------------------------------------------------------
_ARK_ORDER = (0, 2, 4, 1, 3, 5)   # ark's Fq2 slot i holds the coefficient of w^_ARK_ORDER[i]


def from_ark(curve, c):
    """the inverse of pairing_model.to_ark: arkworks' 12 Fq (c0.c0.c0 ... c1.c2.c1) -> pymodel's flat Fq12"""
    cx = ctx(curve)
    a = [0] * 12
    for i, k in enumerate(_ARK_ORDER):
        c0, c1 = c[2 * i], c[2 * i + 1]
        a[k + 6] = c1 % cx.p
        a[k] = (c0 - cx.s * c1) % cx.p
    return a


@lru_cache(maxsize=None)
def _frob_powers(curve, j):
    """(w^(q^j))^k for k = 0..11"""
    cx = ctx(curve)
    F = cx.F
    wq = F.pow([0, 1] + [0] * 10, cx.p ** j)
    out = [F.one]
    for _ in range(11):
        out.append(F.mul(out[-1], wq))
    return out


def frob(curve, a, j):
    """a^(q^j) in the flat ring: sum a_k w^k -> sum a_k (w^(q^j))^k, the a_k in Fq"""
    cx = ctx(curve)
    pw = _frob_powers(curve, j)
    r = [0] * 12
    for k, ak in enumerate(a):
        if ak:
            for i, v in enumerate(pw[k]):
                r[i] += ak * v
    return [v % cx.p for v in r]


def conj(curve, a):
    """the q^6-th power: w -> -w"""
    p = ctx(curve).p
    return [(-v) % p if k & 1 else v % p for k, v in enumerate(a)]


def inv(curve, a):
    """a^-1 = prod_{j=1..11} a^(q^j) / N(a); a != 0"""
    cx = ctx(curve)
    F = cx.F
    t, b = None, a
    for _ in range(11):
        b = frob(curve, b, 1)
        t = b if t is None else F.mul(t, b)
    n = F.mul(a, t)
    assert not any(n[1:]) and n[0], "model: the norm is not in Fq, or a = 0"
    return F.scale(t, pow(n[0], -1, cx.p))


def in_cyclotomic(curve, a):
    """a^(q^4 - q^2 + 1) = 1 and a^(q^6 + 1) = 1, as a^(q^4) a = a^(q^2) and a conj(a) = 1"""
    F = ctx(curve).F
    a2 = frob(curve, a, 2)
    return F.mul(frob(curve, a2, 2), a) == a2 and F.mul(a, conj(curve, a)) == F.one


# ---- slots and checks ----------------------------------------------------------------------------------------------------------------
def _elem_slots(cx, raws):
    return [cx.f.limbs(v) for v in raws]


def _check_elems(cx, want, what, first=0):
    """out slots first .. first + len(want): normalised, below 2 p, residue = want"""
    p, f = cx.p, cx.f

    def check(out):
        for c, w in enumerate(want):
            limbs = [int(x) for x in out[first + c]]
            assert all(x <= MASK for x in limbs[:-1]), "%s: component %d is not normalised: %s" % (what, c, limbs)
            v = f.value(limbs)
            assert v < 2 * p, "%s: component %d = %.4f p, the tower keeps values below 2 p" % (what, c, v / p)
            assert cx.res(v) == w % p, "%s: component %d has the wrong residue (raw value %x)" % (what, c, v)
    return check


def _check_flag(cx, want, what, slot=0):
    def check(out):
        assert [int(x) for x in out[slot]] == cx.flag(want), "%s: flag %s, the model says %d" % (what, list(out[slot])[:2], int(want))
    return check


def _both(*checks):
    def check(out):
        for c in checks:
            c(out)
    return check


def _reps(cx, rng):
    p = cx.p
    return [0, 1, cx.one, p - 1, p, p + 1, 2 * p - 1, rng.randrange(p), p + rng.randrange(p)]


REP_NAMES = ["0", "1", "mont_one", "p-1", "p", "p+1", "2p-1", "random<p", "random>=p"]


def raw_tuples(cx, m, rng, n_random=64):
    """[(label, m raw values below 2 p)]: all at 2 p - 1, all zero, every representative class in every position beside random
    components, then n_random random tuples"""
    p = cx.p
    rnd = lambda: rng.randrange(2 * p)   # noqa: E731
    out = [("all 2p-1", [2 * p - 1] * m), ("all 0", [0] * m), ("all p", [p] * m)]
    for j in range(m):
        for name, s in zip(REP_NAMES, _reps(cx, rng)):
            t = [rnd() for _ in range(m)]
            t[j] = s
            out.append(("component %d = %s" % (j, name), t))
    for i in range(n_random):
        out.append(("random %d" % i, [rnd() for _ in range(m)]))
    return out


def _lazy(cx, residues, rng, mode):
    """raw representatives of residues: mode 0 canonical, 1 every component + p, 2 a random mix; a zero residue as 0 / p"""
    out = []
    for r in residues:
        k = mode if mode < 2 else rng.randrange(2)
        out.append(cx.raw(r, k))
    return out


def named_elements(cx, n2, rng):
    """[(label, raw components)] of an element of n2 Fq2 components (1: Fq2, 3: Fq6, 6: Fq12): the unit, lazy zeros, subfield
    elements, the sparse shapes; zero components alternate between the representatives 0 and p"""
    p = cx.p
    m = 2 * n2

    def masked(live):   # Fq2 positions in `live` random, the rest a lazy zero
        t = []
        for i in range(m):
            t.append(rng.randrange(2 * p) if i // 2 in live else (p if (i + len(live)) & 1 else 0))
        return t
    out = [("the unit", [cx.one] + [0] * (m - 1)), ("the unit + p", [cx.one + p] + [p] * (m - 1)),
           ("lazy zero (all p)", [p] * m), ("lazy zero (0 / p alternating)", [p if i & 1 else 0 for i in range(m)]),
           ("lazy zero (p / 0 alternating)", [0 if i & 1 else p for i in range(m)]),
           ("only c0.c0 (Fq)", [rng.randrange(2 * p)] + [p if i & 1 else 0 for i in range(m - 1)])]
    if n2 == 1:
        out += [("c0 = 0", [0, rng.randrange(2 * p)]), ("c0 = p", [p, rng.randrange(2 * p)]), ("c1 = 0", [rng.randrange(2 * p), 0]),
                ("c1 = p", [rng.randrange(2 * p), p])]
    if n2 == 3:
        for live in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
            out.append(("only Fq2 components %s non-zero" % (live,), masked(live)))
    if n2 == 6:
        # ark order of the Fq2 slots: c0.c0 c0.c1 c0.c2 c1.c0 c1.c1 c1.c2
        out += [("only c0.c0 (Fq2)", masked((0,))), ("only c0 (Fq6), c1 = 0", masked((0, 1, 2))), ("only c1, c0 = 0", masked((3, 4, 5))),
                ("sparse 014", masked((0, 1, 4))), ("sparse 034", masked((0, 3, 4))), ("only c1.c2", masked((5,)))]
    for label, t in out:   # the named shapes hold, by the model alone
        if label.startswith("lazy zero"):
            assert all(v % p == 0 for v in t), label
        if label.startswith("the unit"):
            assert [cx.res(v) for v in t] == [1] + [0] * (m - 1), label
    return out


# ---- models on residues in arkworks' order ------------------------------------------------------------------------------------------
def _t6_flat(cx, c):
    return from_ark(cx.curve, list(c) + [0] * 6)


def _flat_t6(cx, a):
    c = pmod.to_ark(cx.curve, a)
    assert not any(c[6:]), "model: an Fq6 result left Fq6"
    return c[:6]


def _model_alg(cx, form, ops):
    """the expected residues of an algebraic form; ops: the operand residues, flat in slot order"""
    p, F, F2, cv = cx.p, cx.F, cx.F2, cx.curve
    if form.startswith("q_"):
        a = ops[0]
        b = ops[1] if len(ops) > 1 else None
        return [{"q_add": lambda: a + b, "q_sub": lambda: a - b, "q_neg": lambda: -a, "q_dbl": lambda: 2 * a, "q_mul": lambda: a * b,
                 "q_sqr": lambda: a * a}[form]() % p]
    if form.startswith("t2_"):
        a = (ops[0], ops[1])
        b = (ops[2], ops[3]) if len(ops) >= 4 else None
        r = {"t2_add": lambda: F2.add(a, b), "t2_sub": lambda: F2.sub(a, b), "t2_neg": lambda: F2.neg(a),
             "t2_conj": lambda: (a[0], -a[1] % p), "t2_dbl": lambda: F2.add(a, a), "t2_scale": lambda: (a[0] * ops[2] % p, a[1] * ops[2] % p),
             "t2_mul": lambda: F2.mul(a, b), "t2_sqr": lambda: F2.mul(a, a), "t2_mul_by_xi": lambda: F2.mul(a, (cx.s, 1))}[form]()
        return [r[0] % p, r[1] % p]
    if form.startswith("t6_"):
        a = _t6_flat(cx, ops[:6])
        b = _t6_flat(cx, ops[6:12]) if len(ops) >= 12 else None
        v = from_ark(cv, [0, 0, 1, 0] + [0] * 8)
        r = {"t6_add": lambda: F.add(a, b), "t6_sub": lambda: F.sub(a, b), "t6_neg": lambda: F.sub(F.zero, a), "t6_mul": lambda: F.mul(a, b),
             "t6_mul_by_v": lambda: F.mul(a, v)}[form]()
        return _flat_t6(cx, r)
    a = from_ark(cv, ops[:12])
    if form == "t12_mul":
        r = F.mul(a, from_ark(cv, ops[12:24]))
    elif form in ("t12_sqr", "t12_cyc_sqr"):
        r = F.mul(a, a)
    elif form == "t12_conj":
        r = conj(cv, a)
    elif form == "frob":
        r = frob(cv, a, ops[12])
    elif form == "ell":
        r = F.mul(a, _line_elem(cx, ops[12:18], (ops[18], ops[19])))
    else:
        raise KeyError(form)
    return pmod.to_ark(cv, r)


def _line_elem(cx, coeffs, P):
    """the sparse Fq12 element ell() multiplies by: 014 on the M-type twist, 034 on the D-type"""
    p = cx.p
    c0, c1, c2 = coeffs[0:2], coeffs[2:4], coeffs[4:6]
    ark = [0] * 12
    if cx.m_twist:
        ark[0:2] = c0
        ark[2:4] = [c1[0] * P[0] % p, c1[1] * P[0] % p]
        ark[8:10] = [c2[0] * P[1] % p, c2[1] * P[1] % p]
    else:
        ark[0:2] = [c0[0] * P[1] % p, c0[1] * P[1] % p]
        ark[6:8] = [c1[0] * P[0] % p, c1[1] * P[0] % p]
        ark[8:10] = c2
    return from_ark(cx.curve, ark)


ALG_ARITY = {   # form -> (Fq components of the operands, Fq2 components of one operand for the named elements, operands)
    "q_add": (2, 0, 2), "q_sub": (2, 0, 2), "q_neg": (1, 0, 1), "q_dbl": (1, 0, 1), "q_mul": (2, 0, 2), "q_sqr": (1, 0, 1),
    "t2_add": (4, 1, 2), "t2_sub": (4, 1, 2), "t2_neg": (2, 1, 1), "t2_conj": (2, 1, 1), "t2_dbl": (2, 1, 1), "t2_scale": (3, 1, 1),
    "t2_mul": (4, 1, 2), "t2_sqr": (2, 1, 1), "t2_mul_by_xi": (2, 1, 1),
    "t6_add": (12, 3, 2), "t6_sub": (12, 3, 2), "t6_neg": (6, 3, 1), "t6_mul": (12, 3, 2), "t6_mul_by_v": (6, 3, 1),
    "t12_mul": (24, 6, 2), "t12_sqr": (12, 6, 1), "t12_conj": (12, 6, 1), "frob": (12, 6, 1), "ell": (20, 6, 1),
}


def _operand_tuples(cx, m, n2, nops, rng):
    """raw_tuples plus the named elements in every operand position (beside random operands, and against each other)"""
    p = cx.p
    tuples = raw_tuples(cx, m, rng)
    if n2:
        w = 2 * n2
        named = named_elements(cx, n2, rng)
        for pos in range(nops):
            for label, t in named:
                full = [rng.randrange(2 * p) for _ in range(m)]
                full[pos * w:(pos + 1) * w] = t
                tuples.append(("operand %d %s" % (pos, label), full))
        if nops == 2:
            for i, (la, ta) in enumerate(named):
                lb, tb = named[(i * 5 + 3) % len(named)]
                tuples.append(("%s with %s" % (la, lb), ta + tb + [rng.randrange(2 * p) for _ in range(m - 2 * w)]))
                tuples.append(("%s with itself" % la, ta + ta + [rng.randrange(2 * p) for _ in range(m - 2 * w)]))
    return tuples


def _alg_cases(cx, form, rng):
    m, n2, nops = ALG_ARITY[form]
    nout = FORMS[form][2]
    out = []
    variants = [None]
    if form == "frob":
        variants = [1, 2, 3]
    for var in variants:
        for label, t in _operand_tuples(cx, m, n2, nops, rng):
            ops = [cx.res(v) for v in t]
            slots = _elem_slots(cx, t)
            what = "%s %s: %s" % (cx.curve, form, label)
            if var is not None:
                ops = ops[:12] + [var]
                slots = slots[:12] + [cx.flag(var)]
                what += ", j = %d" % var
            want = _model_alg(cx, form, ops)
            assert len(want) == nout
            out.append(Case(slots, _check_elems(cx, want, what), what))
    return out


def _inverse_cases(cx, form, rng):
    """the residue is checked as model.mul(a, got) == 1; a zero element (any lazy zero) gives zero"""
    n = {"q_inverse": 1, "t2_inverse": 2, "t6_inverse": 6, "t12_inverse": 12}[form]
    p, F, cv = cx.p, cx.F, cx.curve
    tuples = raw_tuples(cx, n, rng)
    if n > 1:
        tuples += named_elements(cx, n // 2, rng)
    else:
        tuples += [("the unit", [cx.one]), ("the unit + p", [cx.one + p]), ("minus one", [p - cx.one]), ("minus one + p", [2 * p - cx.one])]
    out = []
    for label, t in tuples:
        res = [cx.res(v) for v in t]
        what = "%s %s: %s" % (cx.curve, form, label)
        zero = not any(res)
        if label.startswith("lazy zero") or label in ("all 0", "all p"):
            assert zero, what

        def check(o, res=res, what=what, zero=zero):
            got = []
            for c in range(n):
                limbs = [int(x) for x in o[c]]
                assert all(x <= MASK for x in limbs[:-1]), "%s: component %d is not normalised" % (what, c)
                v = cx.f.value(limbs)
                assert v < 2 * p, "%s: component %d = %.4f p, the tower keeps values below 2 p" % (what, c, v / p)
                got.append(cx.res(v))
            if zero:
                assert not any(got), "%s: the inverse of zero is zero, got residues %s" % (what, got)
                return
            if n == 1:
                assert res[0] * got[0] % p == 1, "%s: a * got != 1" % what
            elif n == 2:
                assert cx.F2.mul(tuple(res), tuple(got)) == (1, 0), "%s: a * got != 1" % what
            else:
                a = from_ark(cv, res + [0] * (12 - n))
                g = from_ark(cv, got + [0] * (12 - n))
                assert F.mul(a, g) == F.one, "%s: a * got != 1" % what
        out.append(Case(_elem_slots(cx, t), check, what))
    return out


def _flag_cases(cx, form, rng):
    """is_zero / == / equal: the flag is the model's predicate on the residues"""
    p = cx.p
    n = {"q_is_zero": 1, "t12_is_zero": 12, "q_eq": 1, "t2_eq": 2, "equal": 12}[form]
    binary = form in ("q_eq", "t2_eq", "equal")
    out = []

    def add(label, t):
        res = [cx.res(v) for v in t]
        want = res[:n] == res[n:] if binary else not any(res)
        what = "%s %s: %s" % (cx.curve, form, label)
        if label.startswith(("lazy zero", "same residue")):
            assert want, what
        if label.startswith("differs"):
            assert not want, what
        out.append(Case(_elem_slots(cx, t), _check_flag(cx, want, what), what))

    for label, t in raw_tuples(cx, 2 * n if binary else n, rng):
        add(label, t)
    if not binary:
        for i in range(24 if n > 1 else 2):   # every lazy zero: any mix of 0 and p
            add("lazy zero (mix %d)" % i, [p * rng.randrange(2) for _ in range(n)])
        for j in range(n):
            t = [p * rng.randrange(2) for _ in range(n)]
            for name, v in (("1", 1), ("p - 1", p - 1), ("p + 1", p + 1), ("2 p - 1", 2 * p - 1)):
                u = list(t)
                u[j] = v
                add("differs: zero but component %d = %s" % (j, name), u)
        if n > 1:
            for label, t in named_elements(cx, n // 2, rng):
                add(label, t)
    else:
        for i in range(24):
            a = [0] * n if i == 0 else [p - 1] * n if i == 1 else [rng.randrange(p) for _ in range(n)]
            ka = [rng.randrange(2) for _ in range(n)] if i >= 2 else [0] * n   # (0 against p, p - 1 against 2 p - 1)
            kb = [rng.randrange(2) for _ in range(n)] if i >= 2 else [1] * n
            ta = [v + k * p for v, k in zip(a, ka)]
            tb = [v + k * p for v, k in zip(a, kb)]
            add("same residue, other representatives (%d)" % i, ta + tb)
            for j in range(n) if i == 4 else [i % n]:
                u = list(tb)
                u[j] ^= 1   # another residue, still below 2 p (2 p is even)
                add("differs in component %d only (%d)" % (j, i), ta + u)
    return out


# ---- words in, words out ---------------------------------------------------------------------------------------------------------------
def _std_words(cx, residue):
    return cx.f.words(residue * cx.f.Rstd % cx.p)


def _check_words(cx, want_residues, what):
    want = [_std_words(cx, r) for r in want_residues]

    def check(out):
        for c, w in enumerate(want):
            assert [int(x) for x in out[c]] == w, "%s: component %d is not the canonical Montgomery form of the model value" % (what, c)
    return check


def _words_cases(cx, form, rng):
    p = cx.p
    out = []
    if form == "store_gt":   # every representative leaves as the canonical words
        tuples = raw_tuples(cx, 12, rng) + named_elements(cx, 6, rng)
        for label, t in tuples:
            what = "%s store_gt: %s" % (cx.curve, label)
            out.append(Case(_elem_slots(cx, t), _check_words(cx, [cx.res(v) for v in t], what), what))
        return out
    n = 1 if form == "q_std_roundtrip" else 12
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << (p.bit_length() - 1)), pow(cx.f.Rstd, -1, p), cx.R * pow(cx.f.Rstd, -1, p) % p]
    tuples = [("all %x" % v, [v] * n) for v in vals]
    for j in range(n):
        for v in vals[:5]:
            t = [rng.randrange(p) for _ in range(n)]
            t[j] = v
            tuples.append(("component %d = %x" % (j, v), t))
    tuples += [("random %d" % i, [rng.randrange(p) for _ in range(n)]) for i in range(64)]
    for label, t in tuples:
        what = "%s %s: residues %s" % (cx.curve, form, label)
        out.append(Case([_std_words(cx, r) for r in t], _check_words(cx, t, what), what))
    return out


# ---- cyclotomic inputs ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cyclotomic_elements(curve):
    """[(label, flat element)] of the cyclotomic subgroup: three bases f^((q^6 - 1)(q^2 + 1)), their products, conjugates and
    Frobenius images, and 1; each asserted to lie in the subgroup by the model"""
    cx = ctx(curve)
    F, p = cx.F, cx.p
    rng = random.Random("tower/cyc/%s" % curve)
    bases = [F.pow([rng.randrange(p) for _ in range(12)], (p ** 6 - 1) * (p ** 2 + 1)) for _ in range(3)]
    out = [("1", F.one)] + [("g%d" % i, g) for i, g in enumerate(bases)]
    out += [("conj(g%d)" % i, conj(curve, g)) for i, g in enumerate(bases)]
    out += [("g%d g%d" % (i, j), F.mul(bases[i], bases[j])) for i in range(3) for j in range(i, 3)]
    out += [("frob%d(g%d)" % (j, i), frob(curve, g, j)) for i, g in enumerate(bases) for j in (1, 2, 3)]
    out += [("g0 conj(g1)", F.mul(bases[0], conj(curve, bases[1]))), ("g0 g1 g2", F.mul(F.mul(bases[0], bases[1]), bases[2])),
            ("g2 frob1(g0)", F.mul(bases[2], frob(curve, bases[0], 1)))]
    for label, g in out:
        assert in_cyclotomic(curve, g), label
    return out


def _cyc_inputs(cx, rng, n):
    """n (label, raw components): every element canonical, shifted by p, and with a random mix of the two"""
    els = cyclotomic_elements(cx.curve)
    out = []
    i = 0
    while len(out) < n:
        label, g = els[i % len(els)]
        mode = (i // len(els)) % 3
        ark = pmod.to_ark(cx.curve, g)
        out.append(("%s, %s" % (label, ("canonical", "every component + p", "mixed representatives")[mode]), ark, _lazy(cx, ark, rng, mode)))
        i += 1
    return out


def _cyc_cases(cx, form, rng):
    F, cv, r = cx.F, cx.curve, cx.cp.r
    out = []
    if form == "t12_cyc_sqr":
        for label, ark, t in _cyc_inputs(cx, rng, 3 * len(cyclotomic_elements(cv))):
            what = "%s cyc_sqr: %s" % (cv, label)
            a = from_ark(cv, ark)
            out.append(Case(_elem_slots(cx, t), _check_elems(cx, pmod.to_ark(cv, F.mul(a, a)), what), what))
        return out
    if form == "exp_by_x":
        for label, ark, t in _cyc_inputs(cx, rng, 66):
            what = "%s exp_by_x: %s" % (cv, label)
            w = F.pow(from_ark(cv, ark), abs(cx.x))
            if cx.x < 0:
                w = conj(cv, w)
            out.append(Case(_elem_slots(cx, t), _check_elems(cx, pmod.to_ark(cv, w), what), what))
        return out
    if form == "cyc_pow":
        exps = [1, 2, 1 << 32, abs(cx.x), (1 << 64) - 1, 3, (1 << 63), (1 << 32) - 1, (1 << 32) + 1, 36, 30, 18, 12, 6]
        exps += [rng.getrandbits(64) | 1 for _ in range(52)]
        for (label, ark, t), e in zip(_cyc_inputs(cx, rng, len(exps)), exps):
            what = "%s cyc_pow: %s, e = %#x" % (cv, label, e)
            w = F.pow(from_ark(cv, ark), e)
            slots = _elem_slots(cx, t) + [[e & 0xFFFFFFFF, e >> 32] + [0] * (cx.NL - 2)]
            out.append(Case(slots, _check_elems(cx, pmod.to_ark(cv, w), what), what))
        return out
    assert form == "cyc_pow_bits"
    exps = [(0, 0), (0, 1), (0, 256), (1, 1), (1, 256), (2, 2), (2, 256), (r - 1, r.bit_length()), (r - 1, 256), (1 << 255, 256)]
    exps += [((1 << n) - 1, n) for n in (1, 31, 32, 33, 63, 64, 65, 128, 255, 256)]
    exps += [(rng.getrandbits(128), 128) for _ in range(23)] + [(rng.getrandbits(256), 256) for _ in range(22)]
    # only the low nbits bits are the exponent: whatever lies above them in the words is not read
    exps += [((rng.getrandbits(200) << 56) | 0xABCDEF, 56, 0xABCDEF)]
    for (label, ark, t), ex in zip(_cyc_inputs(cx, rng, len(exps)), exps):
        e, nbits = ex[0], ex[1]
        eff = ex[2] if len(ex) > 2 else e
        assert eff == e & ((1 << nbits) - 1)
        what = "%s cyc_pow_bits: %s, e = %#x, %d bits" % (cv, label, e, nbits)
        w = F.pow(from_ark(cv, ark), eff) if eff else F.one
        slots = _elem_slots(cx, t) + [[(e >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [nbits] + [0] * (cx.NL - 9)]
        out.append(Case(slots, _check_elems(cx, pmod.to_ark(cv, w), what), what))
    return out


# ---- the final exponentiation ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def final_exp_bases(curve):
    """[(label, f, f^((q^12 - 1) / r))]: two Miller values and two random elements, the power by F.pow (about half a second each)"""
    cx = ctx(curve)
    cp, F, p = cx.cp, cx.F, cx.p
    G1, G2 = pm.groups(cp)
    rng = random.Random("tower/fe/%s" % curve)
    fs = [("miller(G1, G2)", pmod.miller_loop(curve, cp.g1, cp.g2)),
          ("miller(5 G1, 7 G2)", pmod.miller_loop(curve, G1.mul(cp.g1, 5), G2.mul(cp.g2, 7))),
          ("random a", [rng.randrange(p) for _ in range(12)]), ("random b", [rng.randrange(p) for _ in range(12)])]
    return [(label, f, F.pow(f, (p ** 12 - 1) // cp.r)) for label, f in fs]


def _final_exp_cases(cx, rng):
    """Against F.pow on the four bases; every other input is derived from them with the model (products, powers, conjugates,
    Frobenius images, multiples by subfield elements, which the exponentiation kills), so its expected value is the same
    combination of the bases' powers.  Every lazy zero returns false."""
    F, cv, p = cx.F, cx.curve, cx.p
    bases = final_exp_bases(cv)
    ins = [(label, f, e) for label, f, e in bases]
    for i in range(4):
        for j in range(i, 4):
            (la, fa, ea), (lb, fb, eb) = bases[i], bases[j]
            ins.append(("%s * %s" % (la, lb), F.mul(fa, fb), F.mul(ea, eb)))
    for i, (la, fa, ea) in enumerate(bases):
        k = rng.randrange(1, p)
        ins.append(("%s * an Fq element" % la, F.scale(fa, k), ea))
        k2 = F.from_fq2((rng.randrange(p), rng.randrange(1, p)))
        ins.append(("%s * an Fq2 element" % la, F.mul(fa, k2), ea))
        k6 = _t6_flat(cx, [rng.randrange(p) for _ in range(6)])
        ins.append(("%s * an Fq6 element" % la, F.mul(fa, k6), ea))
        ins.append(("conj(%s)" % la, conj(cv, fa), conj(cv, ea)))
        for j in (1, 2, 3):
            ins.append(("frob%d(%s)" % (j, la), frob(cv, fa, j), frob(cv, ea, j)))
        lb, fb, eb = bases[(i + 1) % 4]
        lc, fc_, ec = bases[(i + 2) % 4]
        ins.append(("%s * %s * %s" % (la, lb, lc), F.mul(F.mul(fa, fb), fc_), F.mul(F.mul(ea, eb), ec)))
        ins.append(("%s^2 * conj(%s)" % (la, lb), F.mul(F.mul(fa, fa), conj(cv, fb)), F.mul(F.mul(ea, ea), conj(cv, eb))))
    ins.append(("the unit", F.one, F.one))
    ins.append(("an Fq6 element (c1 = 0)", _t6_flat(cx, [rng.randrange(p) for _ in range(6)]), F.one))
    ins.append(("an Fq2 element", F.from_fq2((rng.randrange(p), rng.randrange(p))), F.one))
    ins.append(("minus one", F.sub(F.zero, F.one), F.one))
    out = []
    for n, (label, f, e) in enumerate(ins):
        ark = pmod.to_ark(cv, f)
        t = _lazy(cx, ark, rng, n % 3)
        what = "%s final_exp: %s (%s)" % (cv, label, ("canonical", "every component + p", "mixed representatives")[n % 3])
        out.append(Case(_elem_slots(cx, t), _both(_check_elems(cx, pmod.to_ark(cv, e), what), _check_flag(cx, 1, what, slot=12)), what))
    zeros = [[0] * 12, [p] * 12, [p if i & 1 else 0 for i in range(12)], [0 if i & 1 else p for i in range(12)]]
    zeros += [[p * rng.randrange(2) for _ in range(12)] for _ in range(16)]
    for n, t in enumerate(zeros):
        assert all(v % p == 0 for v in t)
        what = "%s final_exp: lazy zero %d (%s)" % (cv, n, "".join("p" if v else "0" for v in t))
        out.append(Case(_elem_slots(cx, t), _both(_check_flag(cx, 0, what, slot=12), _check_elems(cx, [0] * 12, what)), what))
    return out


# ---- the projective line steps ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _g2_multiples(curve, n):
    cp = pm.CURVES[curve]
    G2 = pm.groups(cp)[1]
    pts = [cp.g2]
    for _ in range(n - 1):
        pts.append(G2.add(pts[-1], cp.g2))
    return pts


@lru_cache(maxsize=None)
def _g1_multiples(curve, n):
    cp = pm.CURVES[curve]
    G1 = pm.groups(cp)[0]
    pts = [cp.g1]
    for _ in range(n - 1):
        pts.append(G1.add(pts[-1], cp.g1))
    return pts


def _step_cases(cx, form, rng):
    """dbl_step / add_step on T = (x, y, z), the point (x / z, y / z) of the twist.  The updated T is pymodel's group law.  The three
    coefficients, evaluated at P as ell() places them (the 014 / 034 element), equal pairing_model's untwisted line through the same
    points up to a factor k w^e with k in Fq2: the line l = yP - yT - lam (xP - xT) has, with the untwisting maps x w^-2, y w^-3,
    lam w^-1 of the M-type twist, the value yP - lam2 xP w^-1 + (lam2 x - y) w^-3, and w^3 l has its Fq2 coefficients at w^0, w^2 and
    w^3 -- ark's slots c0.c0, c0.c1, c1.c1 -- so e = 3; with x w^2, y w^3, lam w of the D-type twist l = yP - lam2 xP w + (lam2 x - y)
    w^3 sits at w^0, w^1, w^3 -- c0.c0, c1.c0, c1.c1 -- so e = 0.  k is the projective scaling (-2 y z for a doubling), which the
    final exponentiation kills.  The check divides in the model ring and asserts that the quotient is a non-zero element of Fq2 = <1, w^6>."""
    cv, F, F2, p, cp = cx.curve, cx.F, cx.F2, cx.p, cx.cp
    G2 = pm.groups(cp)[1]
    N = 40
    qs, ps = _g2_multiples(cv, N), _g1_multiples(cv, N)
    out = []

    def case(Taff, z, Raff, P, mode, label):
        """z: the projective scale (an Fq2 residue pair); Raff: the addend, None for a doubling"""
        what = "%s %s: %s" % (cv, form, label)
        if Raff is None:
            line, T3 = pmod._step(cv, Taff, Taff, P)
        else:
            assert Taff[0] != Raff[0], what + ": the addend must be neither T nor -T"
            line, T3 = pmod._step(cv, Taff, Raff, P)
        assert line is not None and T3 == G2.add(Taff, Taff if Raff is None else Raff), what
        res = list(F2.mul(Taff[0], z)) + list(F2.mul(Taff[1], z)) + list(z)
        if Raff is not None:
            res += list(Raff[0]) + list(Raff[1])
        t = _lazy(cx, res, rng, mode)
        line_inv = inv(cv, line)

        def check(o, what=what):
            got = []
            for c in range(12):
                limbs = [int(x) for x in o[c]]
                assert all(x <= MASK for x in limbs[:-1]), "%s: output %d is not normalised" % (what, c)
                v = cx.f.value(limbs)
                assert v < 2 * p, "%s: output %d = %.4f p, the tower keeps values below 2 p" % (what, c, v / p)
                got.append(cx.res(v))
            x, y, zz = (got[0], got[1]), (got[2], got[3]), (got[4], got[5])
            assert zz != (0, 0), "%s: z = 0" % what
            zi = F2.inv(zz)
            assert (F2.mul(x, zi), F2.mul(y, zi)) == T3, "%s: the updated T is not the model's point" % what
            quot = F.mul(F.mul(_line_elem(cx, got[6:12], P), line_inv), _w_inv3(cv) if cx.m_twist else F.one)
            assert any(quot), "%s: the line is zero" % what
            assert not any(v for k, v in enumerate(quot) if k not in (0, 6)), "%s: line / (w^e model line) is not in Fq2: %s" % (what, quot)
        slots = _elem_slots(cx, t)
        out.append(Case(slots, check, what))

    one = (1, 0)
    rz = lambda: (rng.randrange(p), rng.randrange(1, p))   # noqa: E731
    if form == "dbl_step":
        case(qs[0], one, None, ps[0], 0, "T = Q, the first doubling")
        case(qs[0], one, None, ps[0], 1, "T = Q, every component + p")
        for k in range(1, N):
            case(qs[k], one if k < 8 else rz(), None, ps[(k * 7) % N], k % 3, "T = %d Q, %s" % (k + 1, "z = 1" if k < 8 else "z random"))
        for k in range(26):
            case(qs[rng.randrange(N)], rz(), None, ps[rng.randrange(N)], 2, "random %d" % k)
        return out
    neg = lambda Q: (Q[0], F2.neg(Q[1]))   # noqa: E731
    Q = qs[0]
    case(qs[1], one, Q, ps[0], 0, "T = 2 Q + Q, z = 1")
    case(qs[1], one, neg(Q), ps[0], 0, "T = 2 Q - Q (SUB), z = 1")
    for k in range(1, N):
        sub = k % 2 == 0
        case(qs[k], one if k < 6 else rz(), neg(Q) if sub else Q, ps[(k * 3) % N], k % 3,
             "T = %d Q %s Q, %s" % (k + 1, "-" if sub else "+", "z = 1" if k < 6 else "z random"))
    for k in range(24):
        i, j = rng.randrange(2, N), rng.randrange(N)
        if i != j:
            case(qs[i], rz(), qs[j] if k & 1 else neg(qs[j]), ps[rng.randrange(N)], 2, "random %d: %d Q %s %d Q" % (k, i + 1, "+-"[1 - (k & 1)], j + 1))
    # the Frobenius addends that close BN254's loop
    for k in range(0 if cx.m_twist else 8):   # (the D-type map does not land on an M-type twist)
        Qk = qs[k]
        q1 = pmod._frob_twist(cv, Qk, 1)
        q2 = neg(pmod._frob_twist(cv, Qk, 2))
        assert G2.on_curve(q1) and G2.on_curve(q2)
        case(qs[(k + 5) % N], rz(), q1, ps[k], k % 3, "T = %d Q + pi(%d Q)" % ((k + 5) % N + 1, k + 1))
        case(qs[(k + 9) % N], rz(), q2, ps[k + 1], k % 3, "T = %d Q - pi^2(%d Q)" % ((k + 9) % N + 1, k + 1))
    return out


@lru_cache(maxsize=None)
def _w_inv3(curve):
    """w^-3"""
    F = ctx(curve).F
    wi = inv(curve, [0, 1] + [0] * 10)
    return F.mul(wi, F.mul(wi, wi))


def _frob_twist_cases(cx, rng):
    """pi^k on the twist's coordinates: conj^k(x) xi^((q^k - 1) / 3), conj^k(y) xi^((q^k - 1) / 2) (pairing_model._frob_twist)"""
    cv, F2, p = cx.curve, cx.F2, cx.p
    out = []
    for k in (1, 2):
        gx, gy = pmod._frob_twist(cv, ((1, 0), (1, 0)), k)
        tuples = raw_tuples(cx, 4, rng, 32) + [("operand %s" % la, t + [rng.randrange(2 * p), rng.randrange(2 * p)]) for la, t in named_elements(cx, 1, rng)]
        for n, (label, t) in enumerate(tuples):
            r = [cx.res(v) for v in t]
            x, y = (r[0], r[1]), (r[2], r[3])
            if k & 1:
                x, y = (x[0], -x[1] % p), (y[0], -y[1] % p)
            want = list(F2.mul(x, gx)) + list(F2.mul(y, gy))
            if n < 3:
                assert (tuple(want[:2]), tuple(want[2:])) == pmod._frob_twist(cv, ((r[0], r[1]), (r[2], r[3])), k)
            what = "%s frob_twist: %s, k = %d" % (cv, label, k)
            out.append(Case(_elem_slots(cx, t) + [cx.flag(k)], _check_elems(cx, want, what), what))
    return out


def _on_curve_cases(cx, form, rng):
    import subgroup_cases as sc
    cv, p, cp = cx.curve, cx.p, cx.cp
    g2 = form == "g2_on_curve"
    G = pm.groups(cp)[1 if g2 else 0]
    F = G.F
    pts = list((_g2_multiples if g2 else _g1_multiples)(cv, 24))
    comps = (lambda e: list(e)) if g2 else (lambda e: [e])
    cand = [("identity", None)] + [("%d G" % (k + 1), P) for k, P in enumerate(pts)]
    cand += [("torsion point of order %d" % l, T) for l, T in sc.cases(cv, int(g2))[1].items()]
    cand += [("%d G, y + 1" % (k + 1), (P[0], F.add(P[1], F.one))) for k, P in enumerate(pts)]
    cand += [("%d G, x + 1" % (k + 1), (F.add(P[0], F.one), P[1])) for k, P in enumerate(pts)]
    cand += [("%d G, -y" % (k + 1), G.neg(P)) for k, P in enumerate(pts[:8])]
    zero = F.zero
    y0 = sc.sqrt_fq2(G.b, p) if g2 else sc.sqrt_fq(G.b % p, p)
    if y0 is not None:
        cand.append(("(0, sqrt b): x = 0 on the curve", (zero, y0)))
    cand += [("(0, 1)", (zero, F.one)), ("(1, 0)", (F.one, zero)), ("(x of G, 0)", (pts[0][0], zero)), ("(0, y of G)", (zero, pts[0][1]))]
    out = []
    for label, P in cand:
        want = True if P is None else G.on_curve(P)
        if "torsion" in label or label.endswith(" G") or "sqrt b" in label or label == "identity":
            assert want, label
        if "+ 1" in label:
            assert not want, label
        vals = [0] * (4 if g2 else 2) if P is None else comps(P[0]) + comps(P[1])
        what = "%s %s: %s" % (cv, form, label)
        out.append(Case([_std_words(cx, v) for v in vals], _check_flag(cx, want, what), what))
    return out


@lru_cache(maxsize=None)
def cases(curve, form):
    """[Case] of one form on one curve, 65 or more; computed once per process"""
    cx = ctx(curve)
    rng = random.Random("tower/%s/%s" % (curve, form))
    if form in ALG_ARITY:
        out = _alg_cases(cx, form, rng)
    elif form.endswith("_inverse"):
        out = _inverse_cases(cx, form, rng)
    elif form in ("q_is_zero", "t12_is_zero", "q_eq", "t2_eq", "equal"):
        out = _flag_cases(cx, form, rng)
    elif form in ("store_gt", "load_store_gt", "q_std_roundtrip"):
        out = _words_cases(cx, form, rng)
    elif form in ("t12_cyc_sqr", "exp_by_x", "cyc_pow", "cyc_pow_bits"):
        out = _cyc_cases(cx, form, rng)
    elif form == "final_exp":
        out = _final_exp_cases(cx, rng)
    elif form in ("dbl_step", "add_step"):
        out = _step_cases(cx, form, rng)
    elif form == "frob_twist":
        out = _frob_twist_cases(cx, rng)
    elif form in ("g1_on_curve", "g2_on_curve"):
        out = _on_curve_cases(cx, form, rng)
    else:
        raise KeyError(form)
    nin = FORMS[form][1]
    assert len(out) >= 65, (curve, form, len(out))
    assert all(len(c.slots) == nin and all(len(s) == cx.NL for s in c.slots) for c in out), (curve, form)
    return out


def dump_operands(path, run):
    """Write every (curve, form)'s operand tuples, with the outputs run(curve, form, cases) -> uint32 array gave, to one binary file
    for tests/tower_lab_replay.cpp (a stand-alone program that replays them through g16_host_pairing_op, e.g. in a sanitizer build).
    Little-endian uint32 records: curve id, form id, n, operand slots, output slots, NL | n * nin * NL operand words | n * nout * NL
    output words.  Returns the number of records."""
    import numpy as np

    count = 0
    with open(path, "wb") as fh:
        for curve in CURVES:
            for form, (fid, nin, nout) in FORMS.items():
                cs = cases(curve, form)
                NL = ctx(curve).NL
                ops = np.ascontiguousarray(np.array([c.slots for c in cs], dtype="<u4"))
                out = np.ascontiguousarray(run(curve, form, cs), dtype="<u4")
                assert ops.shape == (len(cs), nin, NL) and out.shape == (len(cs), nout, NL)
                fh.write(np.array([fc.CURVE_ID[curve], fid, len(cs), nin, nout, NL], dtype="<u4").tobytes())
                fh.write(ops.tobytes())
                fh.write(out.tobytes())
                count += 1
    return count
