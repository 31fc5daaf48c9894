"""Shared cases and the big-int model of the 30-bit-limb field arithmetic (TEST INFRASTRUCTURE).

Three tiers use this module: the emulator of the generated assembly (tests/fips_asm_emu.py), the host lab entry point
(g16_host_fp30_op) and the device lab (g16_dev_fp30_op).  For a field and a form it yields operand tuples as plain integers (or raw
limb lists where the operation is about limbs) and the EXACT expected integer.

The model knows nothing of fp30.hpp or gen_fips_asm.py beyond the contract their comments state:
  * the moduli come from gen_params.CURVES;
  * limbs are 30 bits wide, NL is the smallest count with R' / p >= 2^9 for R' = 2^(30 NL) (fp30.hpp's header comment);
  * a product form returns V = (T + m p) / R' with T = sum_k x_k y_k (x^2 for sqr) and m = (-T / p) mod R';
  * `*_sK` adds K p - s, `*_x3` adds 6 p - (u + 2 v);
  * results are normalised: V's 30-bit digits, everything from limb NL - 1 upward in the top limb, which must fit 32 bits.

Operand preconditions are the documented ones: normalised limbs, sum_k A_k B_k <= 256 with operands below 16 p for one sweep, 8 p for
two, 4 p for four, and s, u, v < 1.5 p.  One exception, taken from the bound report of g16_host_selftest (G16_SELFTEST_VERBOSE=1,
"largest product T / (R' p)" and "largest operand" of the lane-pair run): the lane-pair squaring hands the one-sweep forms `mul` and
`mul_x3` the operands a0 + a1 and a0 - a1 + 16 p of a 9 p difference, i.e. operands below 18 p and 25 p (the report: "largest
operand 25.0p", "largest product T / (R' p) = 0.717").  Those two forms therefore get extra tuples at (18 p, 25 p); T / (R' p) stays
below 0.72 on BLS12-381's Fq, the tightest field.
"""
import os
import random
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "groth16_amd", "csrc"))
from gen_params import CURVES  # noqa: E402

MASK = (1 << 30) - 1
CURVE_KEY = {"bls12_381": "Bls12_381", "bn254": "Bn254"}
CURVE_ID = {"bls12_381": 0, "bn254": 1}
FIELD_ID = {"fr": 0, "fq": 1}


class Field:
    def __init__(self, curve, which):
        self.curve, self.which = curve, which
        self.p = p = CURVES[CURVE_KEY[curve]]["q" if which == "fq" else "r"]
        nl = 1
        while (1 << (30 * nl)) < (p << 9):   # R' / p >= 2^9
            nl += 1
        self.NL = nl
        self.R = 1 << (30 * nl)
        self.top_shift = 30 * (nl - 1)
        self.NW = (p.bit_length() + 31) // 32
        self.NW += self.NW % 2               # packed form: 32-bit words, an even count (gen_params.field_struct)
        self.Rstd = 1 << (32 * self.NW)
        self.name = "%s_%s" % (curve, which)
        self.struct = "%s%sP" % (CURVE_KEY[curve], "Fq" if which == "fq" else "Fr")   # the name the generated header uses

    # ---- limb views -------------------------------------------------------------------------------------------------------
    def limbs(self, v):
        assert v >= 0
        out = [(v >> (30 * i)) & MASK for i in range(self.NL - 1)] + [v >> self.top_shift]
        assert out[-1] < (1 << 32), "model: the top limb does not fit 32 bits"
        return out

    def value(self, limbs):
        return sum(int(x) << (30 * i) for i, x in enumerate(limbs))

    def words(self, v):
        assert 0 <= v < self.Rstd
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(self.NW)] + [0] * (self.NL - self.NW)

    def from_words(self, w):
        return sum(int(x) << (32 * i) for i, x in enumerate(w[:self.NW]))

    def bound(self, mult):
        """exclusive integer bound `mult` p (mult may be a Fraction)"""
        f = Fraction(mult)
        return -((-f.numerator * self.p) // f.denominator)

    # ---- the Montgomery model ---------------------------------------------------------------------------------------------
    def redc(self, T):
        m = (-T * pow(self.p, -1, self.R)) % self.R
        assert (T + m * self.p) % self.R == 0
        return (T + m * self.p) // self.R


def fields():
    return [Field(c, w) for c in ("bls12_381", "bn254") for w in ("fq", "fr")]


# ---- the product forms (the 32 assembly blocks): name -> (sweeps, squaring, subtraction kind, K) ---------------------------------
PRODUCT_FORMS = {
    "mul": (1, False, None, 0), "sqr": (1, True, None, 0), "mul2": (2, False, None, 0), "mul4": (4, False, None, 0),
    "mul_s2": (1, False, "k", 2), "mul2_s2": (2, False, "k", 2), "mul_s4": (1, False, "k", 4), "mul2_s4": (2, False, "k", 4),
    "mul_s8": (1, False, "k", 8), "mul2_s8": (2, False, "k", 8), "mul_x3": (1, False, "x3", 6), "sqr_x3": (1, True, "x3", 6),
}
FR_FORMS = ("mul", "sqr", "mul2", "mul4")


def product_forms(f):
    return list(PRODUCT_FORMS) if f.which == "fq" else list(FR_FORMS)


def product_operand_bounds(form):
    """multiples of p, one per operand in the block's order: x0 [y0] [x1 y1 ...] [s | u v]"""
    ns, sqr, sub, _ = PRODUCT_FORMS[form]
    per = {1: 16, 2: 8, 4: 4}[ns]
    b = [per] * (ns * (1 if sqr else 2))
    if sub == "k":
        b.append(Fraction(3, 2))
    elif sub == "x3":
        b += [Fraction(3, 2), Fraction(3, 2)]
    return b


def product_model(f, form, ops):
    ns, sqr, sub, K = PRODUCT_FORMS[form]
    if sqr:
        T, rest = ops[0] * ops[0], ops[1:]
    else:
        T, rest = sum(ops[2 * k] * ops[2 * k + 1] for k in range(ns)), ops[2 * ns:]
    V = f.redc(T)
    if sub == "k":
        V += K * f.p - rest[0]
    elif sub == "x3":
        V += 6 * f.p - (rest[0] + 2 * rest[1])
    assert V >= 0
    return V


# ---- special values -----------------------------------------------------------------------------------------------------------
def low_ones(f, bd):
    """every limb but the top equal to 2^30 - 1, the top limb as large as the (exclusive) bound allows"""
    low = (1 << f.top_shift) - 1
    top = (bd - 1) >> f.top_shift
    v = (top << f.top_shift) | low
    if v >= bd:
        v -= 1 << f.top_shift
    return [x for x in (low, v) if 0 <= x < bd]


def specials(f, bd):
    """edge values below the exclusive bound bd, most significant classes first"""
    out = [bd - 1, 0, 1, bd - 2]
    for k in range(16):
        out += [k * f.p + d for d in (0, -1, 1)]
    out += low_ones(f, bd)
    out += [(1 << n) - 1 for n in range(1, bd.bit_length() + 1)]
    seen, res = set(), []
    for v in out:
        if 0 <= v < bd and v not in seen:
            seen.add(v)
            res.append(v)
    return res


def tuples_from(f, bounds, rng, n_random):
    """operand tuples for exclusive integer bounds: all at bound - 1, all zero, one zero, every special value in every operand at
    once and in one operand beside random ones, then n_random seeded random tuples"""
    n = len(bounds)
    sp = [specials(f, b) for b in bounds]
    rnd = lambda: tuple(rng.randrange(b) for b in bounds)   # noqa: E731
    out = [tuple(b - 1 for b in bounds), tuple(0 for _ in bounds)]
    for j in range(n):
        out.append(tuple(0 if i == j else bounds[i] - 1 for i in range(n)))
        t = list(rnd())
        t[j] = 0
        out.append(tuple(t))
    for i in range(max(len(s) for s in sp)):
        out.append(tuple(s[i % len(s)] for s in sp))
        t = list(rnd())
        j = i % n
        t[j] = sp[j][i % len(sp[j])]
        out.append(tuple(t))
    for _ in range(n_random):
        out.append(rnd())
    return out


def product_cases(f, form, seed=1, n_random=64, extended=True):
    """[(operands, expected integer)] for one of the 32 blocks; at least 256 tuples"""
    rng = random.Random("%s/%s/%d" % (f.name, form, seed))
    mults = product_operand_bounds(form)
    ops = tuples_from(f, [f.bound(m) for m in mults], rng, n_random)
    ns, sqr, sub, K = PRODUCT_FORMS[form]
    if sub:   # the subtrahend's own extremes beside every kind of product: the largest s the precondition allows, as a value and per limb
        nprod = len(mults) - (1 if sub == "k" else 2)
        sb = f.bound(Fraction(3, 2))
        for s in [sb - 1] + low_ones(f, sb) + [f.p, f.p - 1, f.p + 1]:
            for prod in (tuple(f.bound(m) - 1 for m in mults[:nprod]), tuple(0 for _ in range(nprod)),
                         tuple(rng.randrange(f.bound(m)) for m in mults[:nprod])):
                ops.append(prod + (s,) * (len(mults) - nprod))
    if extended and form in ("mul", "mul_x3"):   # the lane-pair squaring's operands (module docstring)
        ext = [f.bound(18), f.bound(25)] + [f.bound(m) for m in mults[2:]]
        ops += tuples_from(f, ext, rng, 8)[:48]
    assert len(ops) >= 256
    return [(t, product_model(f, form, t)) for t in ops]


# ---- the field lab: form ids of g16_dev_fp30_op / g16_host_fp30_op (include/g16_mi355x.h) -----------------------------------------
# name -> (id, operand slots, output slots); a slot is NL 32-bit words
LAB = {
    "mul": (0, 2, 1), "sqr": (1, 1, 1), "mul2": (2, 4, 1), "mul4": (3, 8, 1), "mul_s2": (4, 3, 1), "mul2_s2": (5, 5, 1),
    "mul_s4": (6, 3, 1), "mul2_s4": (7, 5, 1), "mul_s8": (8, 3, 1), "mul2_s8": (9, 5, 1), "mul_x3": (10, 4, 1), "sqr_x3": (11, 3, 1),
    "sub2": (20, 2, 1), "sub4": (21, 2, 1), "sub6": (22, 2, 1), "sub8": (23, 2, 1), "sub16": (24, 2, 1), "add_dbl": (25, 2, 1),
    "normalize": (26, 1, 1), "sub_pow2": (27, 3, 1), "unpack_cond_neg": (28, 2, 2), "cond_sub2": (30, 1, 1), "cond_sub4": (31, 1, 1),
    "cond_sub8": (32, 1, 1), "cond_sub16": (33, 1, 1), "weak_reduce32": (34, 1, 1), "canonical_lt2p": (35, 1, 1),
    "canonical_lt8p": (36, 1, 1), "canonical_quick": (37, 1, 1), "neg_canonical": (38, 1, 1), "maybe_zero": (39, 1, 1),
    "is_zero_exact": (40, 1, 1), "to_std": (41, 1, 1), "std_to_r30": (42, 1, 1), "to_packed": (43, 1, 1),
    "fp2x_mul": (50, 4, 2), "fp2x_sqr": (51, 2, 2),
    "pair_mul_v": (60, 4, 2), "pair_sqr_v": (61, 2, 2), "pair_sqr_sub_x3_v": (62, 6, 2), "pair_mul_add_fused": (63, 8, 2),
    "pair_mul_sub": (64, 8, 2), "pair_mul_add_fused_v": (65, 8, 2),
    "acc_chain_g1": (70, 11, 5), "acc_chain_g2": (71, 21, 9), "acc_chain_g2_pair": (72, 21, 9),
    "parked_chain_g1": (73, 11, 5), "parked_chain_g2_pair": (74, 21, 9),
    "inv_plain": (80, 1, 1), "inv": (81, 1, 1), "pair_inv": (82, 2, 2), "jac_dbl_g1": (83, 4, 3), "jac_dbl_g2_pair": (84, 7, 6),
    "aff_pair_g1": (85, 5, 3), "aff_pair_g2_pair": (86, 9, 5),
}
FQ_ONLY = ("fp2x_", "pair_", "acc_", "parked_", "inv", "jac_dbl_", "aff_pair_")
# the lane pair's accumulators, doublings and affine pairs need their lanes: the host twin does not have them
DEVICE_ONLY = ("acc_chain_g2_pair", "parked_chain_g2_pair", "jac_dbl_g2_pair", "aff_pair_g2_pair")
TABLE_FORMS = ("inv_plain", "inv", "pair_inv", "jac_dbl_g1", "jac_dbl_g2_pair", "aff_pair_g1", "aff_pair_g2_pair")   # cases: tests/table_cases.py


def lab_forms(f, host=False):
    out = []
    for name in LAB:
        if host and name in DEVICE_ONLY:
            continue
        if name in PRODUCT_FORMS:
            if name in product_forms(f):
                out.append(name)
        elif name == "sub_pow2":
            if f.which == "fr":
                out.append(name)
        elif name.startswith(FQ_ONLY):
            if f.which == "fq":
                out.append(name)
        else:
            out.append(name)
    return out


def sub_bound(f, kp):
    """b < K p "roughly: b's top limb <= top(K p) - 1" (fp30.hpp, sub<K>): the exclusive value bound that guarantees it"""
    return (kp >> f.top_shift) << f.top_shift


class LabCase:
    """operands: one NL-word list per slot; check(out_slots) raises AssertionError with a message"""
    __slots__ = ("slots", "check", "what")

    def __init__(self, slots, check, what):
        self.slots, self.check, self.what = slots, check, what


def _exact(f, want_limbs, what):
    def check(out):
        assert [int(x) for x in out[0]] == want_limbs, "%s: got %s want %s" % (what, [hex(int(x)) for x in out[0]], [hex(x) for x in want_limbs])
    return check


def _flag(v):
    return [int(v)] + [0] * 15


def fq2_mul(a, b, p):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def _fq2_check(f, want, bound_mult, what):
    lim = f.bound(bound_mult)

    def check(out):
        for c in range(2):
            limbs = [int(x) for x in out[c]]
            assert all(x <= MASK for x in limbs[:-1]), "%s: component %d is not normalised: %s" % (what, c, limbs)
            v = f.value(limbs)
            assert v % f.p == want[c] % f.p, "%s: component %d has the wrong residue (value %x)" % (what, c, v)
            assert v < lim, "%s: component %d = %.3f p, promised < %s p" % (what, c, v / f.p, bound_mult)
    return check


def lab_cases(f, form, seed=1):
    """[LabCase] for a lab form of field f: the product forms reuse product_cases; every other form has its own edge list"""
    p, NL = f.p, f.NL
    rng = random.Random("lab/%s/%s/%d" % (f.name, form, seed))
    L = f.limbs
    out = []

    def vals(bd, n_random=48):
        return specials(f, bd) + [rng.randrange(bd) for _ in range(n_random)]

    if form in PRODUCT_FORMS:
        for t, want in product_cases(f, form, seed):
            out.append(LabCase([L(x) for x in t], _exact(f, L(want), "%s%s" % (form, tuple(hex(x) for x in t))), form))
        return out
    if form.startswith("sub") and form != "sub_pow2" or form == "sub_pow2":
        if form == "sub_pow2":
            ks = list(range(12))
        else:
            ks = [int(form[3:])]
        for k in ks:
            kp = (2 << k) * p if form == "sub_pow2" else k * p
            bb = sub_bound(f, kp)
            ab = f.bound(16) if form != "sub_pow2" else kp
            A, B = vals(ab, 24 if form == "sub_pow2" else 48), vals(bb, 24 if form == "sub_pow2" else 48)
            pairs = [(ab - 1, bb - 1), (0, bb - 1), (ab - 1, 0), (0, 0)] + [(A[i % len(A)], B[(i * 7 + 3) % len(B)]) for i in range(max(len(A), len(B)))]
            if form == "sub_pow2":
                pairs = pairs[:64]
            for a, b in pairs:
                slots = [L(a), L(b)] + ([_flag(k)[:NL]] if form == "sub_pow2" else [])
                out.append(LabCase(slots, _exact(f, L(a + kp - b), "%s(%x, %x, k=%d)" % (form, a, b, k)), form))
        return out
    if form == "add_dbl":
        A = vals(f.bound(16))
        for i, a in enumerate(A):
            b = A[(i * 5 + 1) % len(A)]
            out.append(LabCase([L(a), L(b)], _exact(f, L(a + 2 * b), "add_dbl(%x, %x)" % (a, b)), form))
        return out
    if form == "normalize":
        # raw limbs: every limb but the top up to 2^32 - 4 (the carry into a limb is at most 3, so nothing wraps), the top limb up to 2^31
        hi = (1 << 32) - 4
        raws = [[hi] * (NL - 1) + [1 << 31], [0] * NL, [MASK] * NL, [MASK + 1] * NL, [hi] + [0] * (NL - 1), [0] * (NL - 1) + [1 << 31]]
        raws += [[(1 << n) - 1 if n <= 31 else hi] * (NL - 1) + [(1 << min(n, 31)) - 1] for n in range(1, 33)]
        raws += [[rng.randrange(hi + 1) for _ in range(NL - 1)] + [rng.randrange(1 << 31)] for _ in range(96)]
        for r in raws:
            out.append(LabCase([r], _exact(f, L(f.value(r)), "normalize(%s)" % r), form))
        return out
    if form == "unpack_cond_neg":
        for y in vals(p):
            for flip in (0, 1):
                want = L(2 * p - y if flip else y)

                def check(o, want=want, y=y, flip=flip):
                    assert [int(x) for x in o[0]] == want, "unpack_cond_neg(%x, %d): got %s want %s" % (y, flip, list(o[0]), want)
                    assert [int(x) for x in o[1]] == want, "cond_neg2(unpack(%x), %d): got %s want %s" % (y, flip, list(o[1]), want)
                out.append(LabCase([f.words(y), _flag(flip)[:NL]], check, form))
        return out
    if form.startswith("cond_sub") or form == "weak_reduce32":
        ks = [int(form[8:])] if form.startswith("cond_sub") else [16, 8, 4, 2]
        extra = []
        for k in (2, 4, 8, 16, 1, 3, 31):
            extra += [k * p - 1, k * p, k * p + 1]
        for v in vals(f.bound(32)) + extra:
            w = v
            for k in ks:
                w = w - k * p if w >= k * p else w
            out.append(LabCase([L(v)], _exact(f, L(w), "%s(%x)" % (form, v)), form))
        return out
    if form in ("canonical_lt2p", "canonical_lt8p", "canonical_quick"):
        if form == "canonical_quick":   # any lazy value < 2^18 p whose top limb stays below 2^26
            bd = min(f.bound(1 << 18), 1 << (f.top_shift + 26))
        else:
            bd = f.bound(2 if form == "canonical_lt2p" else 8)
        extra = [k * p + d for k in range(1, 9) for d in (-1, 0, 1)] + [k * p + d for k in (1 << 17, (1 << 18) - 1) for d in (-1, 0, 1)]
        for v in vals(bd) + [x for x in extra if 0 <= x < bd]:
            out.append(LabCase([L(v)], _exact(f, L(v % p), "%s(%x)" % (form, v)), form))
        return out
    if form == "neg_canonical":
        for v in vals(p):
            out.append(LabCase([L(v)], _exact(f, L(p - v), "neg_canonical(%x)" % v), form))
        return out
    if form in ("maybe_zero", "is_zero_exact"):
        bd = f.bound(16)
        near = [k * p + d * (1 << 30) for k in range(16) for d in (1, 2, 1 << (f.top_shift - 30))]   # same low limb as k p, another value
        for v in vals(bd) + [x for x in near if x < bd]:
            if form == "maybe_zero":
                want = any((v - k * p) % (1 << 30) == 0 for k in range(16))
            else:
                want = v % p == 0
            out.append(LabCase([L(v)], _exact(f, _flag(want)[:NL], "%s(%x)" % (form, v)), form))
        return out
    if form in ("to_std", "to_packed"):
        for v in vals(f.bound(16)):
            want = v * f.Rstd * pow(f.R, -1, p) % p if form == "to_std" else v % p
            out.append(LabCase([L(v)], _exact(f, f.words(want), "%s(%x)" % (form, v)), form))
        return out
    if form == "std_to_r30":
        for v in vals(p):
            want = v * f.R * pow(f.Rstd, -1, p) % p
            out.append(LabCase([f.words(v)], _exact(f, f.words(want), "std_to_r30(%x)" % v), form))
        return out
    rinv = pow(f.R, -1, p)
    if form in ("fp2x_mul", "pair_mul_v"):
        bds = [f.bound(8)] * 2 + [f.bound(16)] * 2     # a0 b0 + a1 (16 p - b1): 8 * 16 + 8 * 16 = 256
        for t in tuples_from(f, bds, rng, 64):
            m = fq2_mul(t[0:2], t[2:4], p)
            out.append(LabCase([L(x) for x in t], _fq2_check(f, (m[0] * rinv, m[1] * rinv), Fraction(3, 2), "%s%s" % (form, tuple(hex(x) for x in t))), form))
        return out
    # The squarings multiply a0 + a1 by a0 - a1 + 16 p.  Below 4 p that is 8 * 20 = 160 <= 256 and the promised bound 1.5 p holds.
    # The accumulator squares a difference of up to 9 p (module docstring): operands 18 p x 25 p, T / (R' p) = 450 p / R' > 0.5 on
    # BLS12-381, so for those tuples the bound is the one Montgomery reduction itself gives: below (1 + 450 p / R') p.
    wide = 1 + Fraction(450 * p, f.R)
    if form in ("fp2x_sqr", "pair_sqr_v"):
        for mult, lim in ((4, Fraction(3, 2)), (9, wide)):
            for t in tuples_from(f, [f.bound(mult)] * 2, rng, 64 if mult == 4 else 16):
                m = fq2_mul(t, t, p)
                out.append(LabCase([L(x) for x in t], _fq2_check(f, (m[0] * rinv, m[1] * rinv), lim, "%s%s" % (form, tuple(hex(x) for x in t))), form))
        return out
    if form == "pair_sqr_sub_x3_v":
        for mult, lim in ((4, Fraction(15, 2)), (9, wide + 6)):
            bds = [f.bound(mult)] * 2 + [f.bound(Fraction(3, 2))] * 4
            for t in tuples_from(f, bds, rng, 64 if mult == 4 else 16):
                m = fq2_mul(t[0:2], t[0:2], p)
                want = tuple(m[c] * rinv - (t[2 + c] + 2 * t[4 + c]) for c in range(2))
                out.append(LabCase([L(x) for x in t], _fq2_check(f, want, lim, "%s%s" % (form, tuple(hex(x) for x in t))), form))
        return out
    if form in ("pair_mul_add_fused", "pair_mul_sub", "pair_mul_add_fused_v"):
        # a b +- c d: a0 b0 + a1 (16 p - b1) + two sweeps over c and d; the plain forms need d < 2 p, the prepared (_v) form takes
        # d from 16 p like b:   4 * 16 * 2 + 16 * 2 * 2 = 192,   4 * 16 * 2 + 2 * 16 * 2 = 192
        if form == "pair_mul_add_fused_v":
            bds = [f.bound(4)] * 2 + [f.bound(16)] * 2 + [f.bound(2)] * 2 + [f.bound(16)] * 2
        else:
            bds = [f.bound(4)] * 2 + [f.bound(16)] * 2 + [f.bound(16)] * 2 + [f.bound(2)] * 2
        for t in tuples_from(f, bds, rng, 64):
            ab, cd = fq2_mul(t[0:2], t[2:4], p), fq2_mul(t[4:6], t[6:8], p)
            sgn = -1 if form == "pair_mul_sub" else 1
            want = tuple((ab[c] + sgn * cd[c]) * rinv for c in range(2))
            out.append(LabCase([L(x) for x in t], _fq2_check(f, want, Fraction(3, 2), "%s%s" % (form, tuple(hex(x) for x in t))), form))
        return out
    if form.startswith("acc_chain"):
        return acc_cases(f, form, rng)
    if form.startswith("parked_chain"):
        return parked_cases(f, form, rng)
    if form in TABLE_FORMS:
        import table_cases
        return table_cases.lab_cases(f, form)
    raise KeyError(form)


# ---- the accumulator-level form: a lazy XYZZ accumulator takes a chain of mixed additions -----------------------------------------
def acc_cases(f, form, rng):
    """Acc30 (fp30.hpp) keeps a point as (x, y, zz, zzz) = (X z^2, Y z^3, z^2, z^3) in the R' Montgomery domain, LAZILY: a coordinate
    may be any representative r + k p below its bound (x < 7.5 p, y < 3.5 p, zz and zzz < 1.8 p).  The mixed addition tests
    H = px zz - x and R = py zzz - y for zero through maybe_zero / is_zero_exact, where a zero shows up as SOME multiple k p: with
    x = r + kx p (kx = 0..6) and y = r + ky p (ky = 0..2) every admissible k is produced, in H and in R, for P + P (the doubling
    branch) and P - P (the identity).  Also: the identity accumulator, identity points in the chain, and random chains.  Expected:
    pymodel's group law on affine points; the device's XYZZ result is compared as a canonical affine point."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pymodel
    cp = pymodel.CURVES[f.curve]
    g2 = form != "acc_chain_g1"
    G = pymodel.groups(cp)[1 if g2 else 0]
    F, p, NL = G.F, f.p, f.NL
    C = 2 if g2 else 1
    comps = (lambda e: list(e)) if g2 else (lambda e: [e])
    elem = (lambda c: (c[0], c[1])) if g2 else (lambda c: c[0])
    gen = cp.g2 if g2 else cp.g1
    pts = [None, gen]
    for _ in range(40):
        pts.append(G.add(pts[-1], gen))
    rinv = pow(f.R, -1, p)

    def lazy(e, ks):       # Montgomery form, component c as the representative r + ks[c] p
        return [f.limbs(c * f.R % p + k * p) for c, k in zip(comps(e), ks)]

    def accumulator(A, z, kx, ky):
        if A is None:
            return [[0] * NL] * (4 * C), 1
        zz = F.sqr(z)
        zzz = F.mul(zz, z)
        return lazy(F.mul(A[0], zz), kx) + lazy(F.mul(A[1], zzz), ky) + lazy(zz, [0] * C) + lazy(zzz, [0] * C), 0

    def scale():
        return elem([rng.randrange(1, p) for _ in range(C)])

    def case(A, z, kx, ky, chain, kp, what):
        acc, inf = accumulator(A, z, kx, ky)
        flags = [inf, len(chain)] + [1 if Q is None else 0 for Q in chain] + [0] * 3
        slots = acc + [(flags + [0] * NL)[:NL]]
        want = A
        for j in range(3):
            Q = chain[j] if j < len(chain) else None
            if Q is None:
                slots += [[0] * NL] * (2 * C)
            else:   # affine points enter below 2 p: canonical, or canonical + p
                slots += lazy(Q[0], [kp] * C) + lazy(Q[1], [kp] * C)
                want = G.add(want, Q)

        def check(out, want=want, what=what):
            got_inf = int(out[4 * C][0])
            if want is None:
                assert got_inf == 1, "%s: expected the identity, got a point" % what
                return
            assert got_inf == 0, "%s: got the identity, expected %s" % (what, want)
            v = [[f.from_words(out[e * C + c]) for c in range(C)] for e in range(4)]
            assert all(x < p for e in v for x in e), "%s: a coordinate is not canonical" % what
            x, y, zz, zzz = [elem([c * rinv % p for c in e]) for e in v]
            got = (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))
            assert got == want, "%s: got %s want %s" % (what, got, want)
        return LabCase(slots, check, form)

    out = []
    ks = [[k] * C for k in range(7)] + ([[0, 6], [5, 1]] if g2 else [])
    kys = [[k] * C for k in range(3)] + ([[0, 2]] if g2 else [])
    i = 0
    for kx in ks:
        for ky in kys:
            P = pts[1 + i % 20]
            i += 1
            for sign, name in ((1, "P + P"), (-1, "P - P")):
                A = P if sign == 1 else G.neg(P)
                out.append(case(A, scale(), kx, ky, [P], i % 2, "%s %s, x + %s p, y + %s p" % (form, name, kx, ky)))
    P, Q, S = pts[3], pts[7], pts[11]
    out.append(case(None, None, None, None, [], 0, form + " identity, empty chain"))
    out.append(case(None, None, None, None, [P], 0, form + " identity + P"))
    out.append(case(None, None, None, None, [P, P], 1, form + " identity + P + P"))
    out.append(case(None, None, None, None, [P, P, G.neg(pts[6])], 0, form + " identity + P + P - 2 P"))
    out.append(case(None, None, None, None, [None, P, None], 0, form + " identity + O + P + O"))
    out.append(case(Q, scale(), ks[3], kys[1], [None, None, None], 0, form + " Q + O + O + O"))
    out.append(case(Q, scale(), ks[6], kys[2], [None, S, None], 1, form + " Q + O + S + O"))
    out.append(case(Q, scale(), ks[0], kys[0], [G.neg(Q), S, S], 0, form + " Q - Q + S + S"))
    for n in range(24):
        A = pts[1 + rng.randrange(40)]
        chain = [pts[rng.randrange(41)] for _ in range(1 + n % 3)]
        out.append(case(A, scale(), ks[rng.randrange(len(ks))], kys[rng.randrange(len(kys))], chain, n % 2, "%s random chain %d" % (form, n)))
    return out


# ---- the bucket pass's own accumulator: parked coordinates, signed additions, a sign that gather() resolves ------------------------
def parked_cases(f, form, rng):
    """AccParked (fp30.hpp) as bucket_accumulate30_kernel runs it.  The parked coordinates are lazy like Acc30's (x < 7.5 p, y < 3.5 p,
    zz and zzz < 1.8 p) and may be those of -A (`neg`): a hot-path addition leaves the negated sum, so the next point enters with its
    sign flipped -- together with the signed digit's own sign (`minus`) -- and gather() negates y once, at the flush.  The cold
    branches (first point, doubling) keep the sign they find, a cancellation leaves `neg` behind beside the identity flag and the
    first point after it must reset it.  Points come as the window table holds them: canonical, x and y packed in words.

    A case is written down by the point the accumulator REPRESENTS (A), the initial neg, and the chain [(Q, minus)]; the tuple holds
    the coordinates as parked, i.e. those of -A when neg is set.  Expected: pymodel's group law, A + sum +-Q, compared as a canonical
    affine point.  Every step a case names a doubling or a cancellation is asserted to be one with the model alone."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pymodel
    cp = pymodel.CURVES[f.curve]
    g2 = form != "parked_chain_g1"
    G = pymodel.groups(cp)[1 if g2 else 0]
    F, p, NL = G.F, f.p, f.NL
    C = 2 if g2 else 1
    comps = (lambda e: list(e)) if g2 else (lambda e: [e])
    elem = (lambda c: (c[0], c[1])) if g2 else (lambda c: c[0])
    gen = cp.g2 if g2 else cp.g1
    pts = [None, gen]
    for _ in range(40):
        pts.append(G.add(pts[-1], gen))
    rinv = pow(f.R, -1, p)

    def lazy(e, ks):       # Montgomery form, component c as the representative r + ks[c] p
        return [f.limbs(c * f.R % p + k * p) for c, k in zip(comps(e), ks)]

    def packed(e):         # Montgomery form, canonical, in the packed form's words
        return [f.words(c * f.R % p) for c in comps(e)]

    def scale():
        return elem([rng.randrange(1, p) for _ in range(C)])

    def signed(Q, minus):
        return G.neg(Q) if (minus and Q is not None) else Q

    def case(A, neg, kx, ky, chain, what, steps=(), kz=0):
        """chain: [(Q or None, minus)]; steps: what each step must be by the model -- "dbl", "cancel", "first" or None;
        kz = 1: zz and zzz as r + p, with a scale whose residues leave that below 1.8 p"""
        if A is None:
            acc, inf = [[0] * NL] * (4 * C), 1
        else:
            Ap = G.neg(A) if neg else A
            while True:
                z = scale()
                zz = F.sqr(z)
                zzz = F.mul(zz, z)
                if not kz or all(5 * (c * f.R % p + p) < 9 * p for e in (zz, zzz) for c in comps(e)):
                    break
            acc, inf = lazy(F.mul(Ap[0], zz), kx) + lazy(F.mul(Ap[1], zzz), ky) + lazy(zz, [kz] * C) + lazy(zzz, [kz] * C), 0
        flags = [inf, int(neg), len(chain)] + [1 if j < len(chain) and chain[j][0] is None else 0 for j in range(3)]
        flags += [int(chain[j][1]) if j < len(chain) else 0 for j in range(3)]
        slots = acc + [(flags + [0] * NL)[:NL]]
        want = A
        for j in range(3):
            Q, minus = chain[j] if j < len(chain) else (None, 0)
            if Q is None:
                slots += [[0] * NL] * (2 * C)
                assert j >= len(steps) or steps[j] is None, what
                continue
            slots += packed(Q[0]) + packed(Q[1])
            sQ = signed(Q, minus)
            if j < len(steps) and steps[j] is not None:   # the collision the case is named after really happens, by the model alone
                if steps[j] == "dbl":
                    assert want is not None and sQ == want, "%s: step %d is no doubling" % (what, j)
                elif steps[j] == "cancel":
                    assert want is not None and sQ == G.neg(want) and G.add(want, sQ) is None, "%s: step %d is no cancellation" % (what, j)
                elif steps[j] == "first":
                    assert want is None, "%s: step %d does not meet the identity" % (what, j)
                else:
                    assert steps[j] == "hot" and want is not None and sQ[0] != want[0], "%s: step %d is no plain addition" % (what, j)
            want = G.add(want, sQ)

        def check(out, want=want, what=what):
            got_inf = int(out[4 * C][0])
            if want is None:
                assert got_inf == 1, "%s: expected the identity, got a point" % what
                return
            assert got_inf == 0, "%s: got the identity, expected %s" % (what, want)
            v = [[f.from_words(out[e * C + c]) for c in range(C)] for e in range(4)]
            assert all(x < p for e in v for x in e), "%s: a coordinate is not canonical" % what
            x, y, zz, zzz = [elem([c * rinv % p for c in e]) for e in v]
            got = (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))
            assert got == want, "%s: got %s want %s" % (what, got, want)
        return LabCase(slots, check, form)

    out = []
    ks = [[k] * C for k in range(7)] + ([[0, 6], [5, 1]] if g2 else [])
    kys = [[k] * C for k in range(3)] + ([[0, 2]] if g2 else [])
    k0, y0 = ks[0], kys[0]
    i = 0
    # P + P and P - P for every admissible representative, from either parked sign and with either digit sign: the point is chosen
    # so that the SIGNED addition meets +-(the represented point)
    for kx in ks:
        for ky in kys:
            for neg in (0, 1):
                for minus in (0, 1):
                    A = pts[1 + i % 20]
                    i += 1
                    tail = "neg = %d, minus = %d, x + %s p, y + %s p" % (neg, minus, kx, ky)
                    out.append(case(A, neg, kx, ky, [(signed(A, minus), minus)], "%s A + A (doubling), %s" % (form, tail), ["dbl"]))
                    out.append(case(A, neg, kx, ky, [(signed(G.neg(A), minus), minus)], "%s A - A (cancellation), %s" % (form, tail), ["cancel"]))
    P, Q, S, T = pts[3], pts[7], pts[11], pts[13]
    for neg in (0, 1):   # (an identity accumulator keeps the neg a flush or a cancellation left behind)
        for minus in (0, 1):
            t = "neg = %d, minus = %d" % (neg, minus)
            out.append(case(None, neg, None, None, [(P, minus)], "%s first point into the identity, %s" % (form, t), ["first"]))
            out.append(case(None, neg, None, None, [(P, minus), (Q, 1 - minus)], "%s first point then a hot addition, %s" % (form, t), ["first", "hot"]))
            # the cold branch keeps neg: the addition after a doubling must still take the parked sign
            out.append(case(P, neg, ks[2], kys[1], [(signed(P, minus), minus), (Q, minus)],
                            "%s doubling then an addition, %s" % (form, t), ["dbl", "hot"]))
            out.append(case(P, neg, ks[5], kys[2], [(signed(P, minus), minus), (Q, 1 - minus), (S, minus)],
                            "%s doubling then two additions, %s" % (form, t), ["dbl", "hot", "hot"]))
            # a cancellation leaves neg behind: the first point after it must reset it
            out.append(case(P, neg, ks[1], kys[0], [(signed(G.neg(P), minus), minus), (Q, minus)],
                            "%s cancellation then an addition, %s" % (form, t), ["cancel", "first"]))
            out.append(case(P, neg, ks[4], kys[1], [(signed(G.neg(P), minus), minus), (Q, 1 - minus), (S, minus)],
                            "%s cancellation then two additions, %s" % (form, t), ["cancel", "first", "hot"]))
            # a doubling / a cancellation reached after one hot addition (neg has toggled once)
            PQ = G.add(P, signed(Q, minus))
            out.append(case(P, neg, ks[3], kys[2], [(Q, minus), (signed(PQ, minus), minus)],
                            "%s hot addition then a doubling, %s" % (form, t), ["hot", "dbl"]))
            out.append(case(P, neg, ks[6], kys[0], [(Q, minus), (signed(G.neg(PQ), 1 - minus), 1 - minus), (T, minus)],
                            "%s hot addition, a cancellation, then a first point, %s" % (form, t), ["hot", "cancel", "first"]))
            # gather() after an odd and an even number of hot additions
            for n in (1, 2, 3):
                chain = [((Q, S, T)[j], (minus + j) % 2) for j in range(n)]
                out.append(case(P, neg, ks[n], kys[n - 1], chain, "%s %d hot additions, %s" % (form, n, t), ["hot"] * n))
            # identity points inside the chain are skipped and do not toggle anything
            out.append(case(P, neg, k0, y0, [(None, minus), (Q, minus), (None, 1 - minus)], "%s O, Q, O, %s" % (form, t)))
            out.append(case(P, neg, k0, y0, [(Q, minus), (None, 1), (S, 1 - minus)], "%s Q, O, S, %s" % (form, t)))
            out.append(case(P, neg, k0, y0, [(None, 1), (None, 0), (None, 1)], "%s O, O, O, %s" % (form, t)))
            out.append(case(None, neg, None, None, [(None, minus), (None, minus), (Q, minus)], "%s identity + O + O + Q, %s" % (form, t), [None, None, "first"]))
            # zz, zzz in the upper part of their range (r + p < 1.8 p): U2 - x and S2 - y from the largest admissible operands
            tz = "zz + p, zzz + p, " + t
            out.append(case(P, neg, ks[6], kys[2], [(signed(P, minus), minus)], "%s A + A (doubling), %s" % (form, tz), ["dbl"], kz=1))
            out.append(case(P, neg, ks[6], kys[2], [(signed(G.neg(P), minus), minus)], "%s A - A (cancellation), %s" % (form, tz), ["cancel"], kz=1))
            out.append(case(P, neg, ks[6], kys[2], [(Q, minus), (S, 1 - minus)], "%s two hot additions, %s" % (form, tz), ["hot", "hot"], kz=1))
    out.append(case(None, 0, None, None, [], form + " identity, empty chain"))
    out.append(case(P, 1, ks[6], kys[2], [], form + " empty chain, neg = 1: gather() alone"))
    for n in range(32):
        A = pts[1 + rng.randrange(40)]
        chain = [(pts[rng.randrange(41)], rng.randrange(2)) for _ in range(1 + n % 3)]
        out.append(case(A, rng.randrange(2), ks[rng.randrange(len(ks))], kys[rng.randrange(len(kys))], chain, "%s random chain %d" % (form, n)))
    return out
