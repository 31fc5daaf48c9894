"""Shared by the subgroup-membership tests (both tiers): per curve and per group a list of points with the verdict the big-int
model gives them.  The ground truth is multiplication by r: a curve point P is in the prime-order subgroup iff [r]P is the
identity.  pymodel.Group.mul reduces its scalar modulo the group's `r`, which would make [r]P the identity for every P, so the
groups here are built with a modulus no scalar of this file reaches."""
import functools

import numpy as np

import pymodel as pm
from helpers import g1_to_arr, g2_to_arr

NAMES = ["bls12_381", "bn254"]
BLS_X = -0xD201000000010000
BN_X = 4965661367192848881
# primes below 2^20 that the issue expects in each cofactor (the helper finds them by trial division and asserts these)
EXPECTED_PRIMES = {("bls12_381", 0): [3, 11, 10177, 859267], ("bls12_381", 1): [13, 23, 2713, 11953, 262069],
                   ("bn254", 0): [], ("bn254", 1): [10069]}


def model_groups(cp):
    """(G1, G2) whose mul / jmul take the scalar as it is"""
    big = 1 << 4096
    return pm.Group(pm.Fq1(cp.q), cp.b1, big), pm.Group(pm.Fq2(cp.q), cp.b2, big)


def cofactor(name, g2):
    """#E(Fq) / r and #E'(Fq2) / r from the curve families' polynomials (checked on random curve points in cases())"""
    cp = pm.CURVES[name]
    if name == "bls12_381":
        x = BLS_X
        if not g2:
            assert (x - 1) ** 2 % 3 == 0
            return (x - 1) ** 2 // 3
        h = x**8 - 4 * x**7 + 5 * x**6 - 4 * x**4 + 6 * x**3 - 4 * x**2 - 4 * x + 13
        assert h % 9 == 0
        return h // 9
    return 2 * cp.q - cp.r if g2 else 1   # BN: #E(Fq) = r, #E'(Fq2) = r (2q - r)


def small_primes_of(h, bound=1 << 20):
    out, d = [], 2
    while d < bound:
        if h % d == 0:
            out.append(d)
            while h % d == 0:
                h //= d
        d += 1 if d == 2 else 2
    return out


def sqrt_fq(a, q):
    """q = 3 mod 4; None for a non-square"""
    s = pow(a, (q + 1) // 4, q)
    return s if s * s % q == a % q else None


def sqrt_fq2(a, q):
    a0, a1 = a[0] % q, a[1] % q
    if a1 == 0:
        s = sqrt_fq(a0, q)
        if s is not None:
            return (s, 0)
        return (0, sqrt_fq(-a0 % q, q))   # -a0 is a square when a0 is not (q = 3 mod 4), and u^2 = -1
    n = sqrt_fq((a0 * a0 + a1 * a1) % q, q)
    if n is None:
        return None
    inv2 = pow(2, q - 2, q)
    for cand in ((a0 + n) * inv2 % q, (a0 - n) * inv2 % q):
        x0 = sqrt_fq(cand, q)
        if x0:
            x1 = a1 * pow(2 * x0, q - 2, q) % q
            return (x0, x1)
    return None


def random_curve_point(G, cp, g2, rng):
    """a point of the whole curve group (no cofactor clearing)"""
    q = cp.q
    while True:
        if g2:
            x = (rng.field(q), rng.field(q))
            y = sqrt_fq2(G.F.add(G.F.mul(G.F.sqr(x), x), G.b), q)
        else:
            x = rng.field(q)
            y = sqrt_fq((x * x * x + G.b) % q, q)
        if y is not None:
            P = (x, y) if rng.next() & 1 else (x, G.F.neg(y))
            assert G.on_curve(P)
            return P


def model_flag(G, cp, P):
    """the ABI's byte from the model: 2 off the curve, 1 if [r]P is the identity, else 0"""
    if not G.on_curve(P):
        return 2
    return 1 if G.mul(P, cp.r) is None else 0


@functools.lru_cache(maxsize=None)
def cases(name, g2):
    """[(label, affine point or None, flag)] and the torsion points {l: T} of one group"""
    cp = pm.CURVES[name]
    G = model_groups(cp)[g2]
    gen = cp.g2 if g2 else cp.g1
    rng = pm.SplitMix64(0x5B6 + 2 * NAMES.index(name) + g2)
    h = cofactor(name, g2)
    out = [("identity", None)]
    members = [G.mul(gen, k) for k in [1, cp.r - 1] + [rng.field(cp.r - 1) + 1 for _ in range(6)]]
    out += [(f"member{i}", P) for i, P in enumerate(members)]
    randoms = [random_curve_point(G, cp, g2, rng) for _ in range(8)]
    assert G.mul(randoms[0], cp.r * h) is None, "the cofactor is wrong"
    out += [(f"random{i}", P) for i, P in enumerate(randoms)]
    primes = small_primes_of(h)
    assert primes == EXPECTED_PRIMES[(name, int(g2))], primes
    torsion = {}
    for l in primes:
        # [r h / l^e] R lies in the l-part of the curve group (l^e || h); multiplying on by l until the next step would reach the
        # identity leaves order exactly l.  ([r h / l] R alone is always the identity where that part is not cyclic: l = 11 in
        # BLS12-381's G1 is Z_11 x Z_11.)
        le = l
        while h % (le * l) == 0:
            le *= l
        T = None
        for _ in range(64):
            T = G.mul(random_curve_point(G, cp, g2, rng), cp.r * h // le)
            if T is not None:
                break
        assert T is not None, l
        while G.mul(T, l) is not None:
            T = G.mul(T, l)
        assert G.mul(T, l) is None   # l is prime and T is not the identity: the order is exactly l
        torsion[l] = T
        out.append((f"order{l}", T))
    for k, (l, T) in enumerate(torsion.items()):
        out.append((f"member+order{l}", G.add(members[k % len(members)], T)))
    off = (members[2][0], G.F.add(members[2][1], G.F.one))
    out.append(("off_curve", off))
    flagged = [(label, P, model_flag(G, cp, P)) for label, P in out]
    for label, P, f in flagged:
        if label == "identity" or label.startswith("member") and "+" not in label:
            assert f == 1, label
        elif label == "off_curve":
            assert f == 2, label
        elif label.startswith("random"):
            assert f == (1 if h == 1 else 0), label   # BN254 G1 is the whole curve
        else:
            assert f == 0, label
    return flagged, torsion


def to_arr(points, name, g2):
    cp = pm.CURVES[name]
    return g2_to_arr(points, cp) if g2 else g1_to_arr(points, cp)


def case_arrays(name, g2):
    """(labels, (n, words) uint64 points, uint8 flags) of cases()"""
    flagged, _ = cases(name, g2)
    return [c[0] for c in flagged], to_arr([c[1] for c in flagged], name, g2), np.array([c[2] for c in flagged], dtype=np.uint8)
