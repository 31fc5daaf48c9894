"""Phase 1: the cases the CPU and GPU tiers share (TEST INFRASTRUCTURE, no GPU), built on table_cases.py, srs_cases.py and
ceremony_cases.py.

Scalar multiplication.  The expected value of k P comes from table_cases.Model -- a plain affine law with a = 0 that takes ANY
(x, y) and reduces nothing modulo a group order -- by double-and-add over the bits of k, so the points may leave the prime-order
subgroup and the curve.  The device kernel reads a scalar as 64 signed 4-bit digits: recode() is the reference recoding (the nibbles
of k + 0x88..8, minus 8 each) and asserts sum d_j 16^j == k for every scalar used here.

Contributions.  A contribution with secrets (t', a', b') to the model SRS of (t, a, b) is the model SRS of (t t', a a', b b'); the
public record is (t' g2, a' g2, b' g2).  check_cases() tampers with that in the model, where every discrete logarithm is known."""
import functools

import numpy as np

import ceremony_cases as cc
import pymodel as pm
import srs_cases as sc
import table_cases as tc
from helpers import g2_to_arr, ints_to_mont

DIGITS = 64
BIAS = int("8" * DIGITS, 16)
SHAPE, TAU_RATIO, ALPHA_RATIO, BETA_RATIO = "SHAPE", "TAU_RATIO", "ALPHA_RATIO", "BETA_RATIO"
PUB_FIELDS = ("tau_g2", "alpha_g2", "beta_g2")


def recode(k: int):
    """the 64 signed digits (least significant first, each in [-8, 7]) the kernel reads k as"""
    kb = k + BIAS
    assert 0 <= k and kb < 1 << (4 * DIGITS), "k + 0x88..8 must fit 256 bits"
    d = [((kb >> (4 * j)) & 15) - 8 for j in range(DIGITS)]
    assert all(-8 <= x <= 7 for x in d) and sum(x << (4 * j) for j, x in enumerate(d)) == k
    return d


@functools.lru_cache(maxsize=None)
def scalars(curve: str):
    """[(label, k)], every k in [0, r) and recoded once"""
    r = pm.CURVES[curve].r
    out = [("%d" % k, k) for k in (0, 1, 2, 7, 8, 9, 15, 16, 17)]
    out += [("r-1", r - 1), ("r-2", r - 2), ("(r-1)/2", (r - 1) // 2), ("(r+1)/2", (r + 1) // 2)]
    for w in range(1, DIGITS):
        if (1 << (4 * w)) < r:
            out += [("2^%d" % (4 * w), 1 << (4 * w)), ("2^%d-1" % (4 * w), (1 << (4 * w)) - 1)]
    out.append(("0x88..8 mod r", BIAS % r))
    out.append(("0x088..8", int("8" * (DIGITS - 1), 16)))                       # every nibble 8 below the top one
    out.append(("0x0ff..f", int("f" * (DIGITS - 1), 16)))                       # a carry through every window
    out.append(("0x077..7", int("7" * (DIGITS - 1), 16)))                       # every digit of the recoding +7, the top one 0
    out.append(("+-8 alternating", sum((8 if j % 2 == 0 else -8) << (4 * j) for j in range(DIGITS - 1))))
    out.append(("1 over -8s", (9 << (4 * (DIGITS - 1))) - BIAS))               # the recoding's digits: -8 everywhere, 1 on top
    for label, k in out:
        assert 0 <= k < r, label
        recode(k)
    d = dict(out)
    assert recode(d["1 over -8s"]) == [-8] * (DIGITS - 1) + [1] and recode(d["0x077..7"]) == [7] * (DIGITS - 1) + [0]
    return out


SMALL = ("0", "1", "2", "7", "8", "9", "16", "17", "r-1", "(r+1)/2", "0x088..8", "1 over -8s")


@functools.lru_cache(maxsize=None)
def expected(curve: str, g2: bool, P, k: int):
    """k P by double-and-add in the affine model (no reduction of k, any point)"""
    m = tc.model(curve, g2)
    acc = None
    for i in range(k.bit_length() - 1, -1, -1):
        acc = m.dbl(acc)
        if (k >> i) & 1:
            acc = m.add(acc, P)
    return acc


@functools.lru_cache(maxsize=None)
def smul_cases(curve: str, g2: bool):
    """[(label, P, k)]: every scalar on a rotating point (multiples of the generator, the identity, one point repeated), then every
    point of table_cases.pool -- orders 2, 3, 4 and off-curve points among them -- under the SMALL scalars"""
    m = tc.model(curve, g2)
    mult = dict(tc.point_classes(curve, g2))["multiple of the generator"]
    sc_ = scalars(curve)
    rot = [mult[0], mult[4], None, mult[7], mult[7], mult[11]]
    out = [("%s * rot%d" % (label, i % len(rot)), rot[i % len(rot)], k) for i, (label, k) in enumerate(sc_)]
    small = [(label, k) for label, k in sc_ if label in SMALL]
    assert len(small) == len(SMALL)
    for j, P in enumerate(tc.pool(curve, g2)):
        out += [("%s * pool%d" % (label, j), P, k) for label, k in small]
    # the premises of the slow path: some case adds a point to itself, some case adds a point to its negative, inside the window walk
    three = dict(tc.point_classes(curve, g2))["(0, y)"][0]
    assert m.add(m.dbl(three), three) is None and m.add(m.chain(three, 2), three) == m.dbl(three)
    return out


def small_order_points(curve: str, g2: bool):
    """the points whose multiples repeat within the table 1P .. 8P"""
    cls = dict(tc.point_classes(curve, g2))
    pts = list(cls["(x, 0)"]) + list(cls["(0, y)"])
    if g2:
        pts += list(cls["order 4"])
    return pts


def smul_arrays(curve: str, g2: bool, cases):
    """(points, scalars, expected) as the ABI's arrays"""
    m = tc.model(curve, g2)
    cp = pm.CURVES[curve]
    pts = np.array([tc.abi_words(m, P) for _, P, _ in cases], dtype=np.uint64)
    ks = ints_to_mont([k for _, _, k in cases], cp.r, 4)
    want = np.array([tc.abi_words(m, expected(curve, g2, P, k)) for _, P, k in cases], dtype=np.uint64)
    return pts, np.ascontiguousarray(ks), want


# ---- contributions -------------------------------------------------------------------------------------------------------------
def contribution_secrets(cp, seed: int = 77):
    rng = pm.SplitMix64(seed)
    return tuple(rng.field(cp.r - 1) + 1 for _ in range(3))


def contributed(cp, sec, mine):
    """the secrets after a contribution (tau', alpha', beta') to an SRS of `sec`"""
    t, a, b = mine
    return dict(sec, tau=sec["tau"] * t % cp.r, alpha=sec["alpha"] * a % cp.r, beta=sec["beta"] * b % cp.r)


def model_pub(cp, sec, mine):
    G2 = pm.groups(cp)[1]
    return [G2.mul(sec["g2"], s) for s in mine]


def pub_to_arrays(g, cp, pub):
    return g.TauContribution(cp.name, *[g2_to_arr([P], cp)[0].copy() for P in pub])


def assert_srs_equal(got, want, label=""):
    for f in cc.SRS_ARRAYS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.shape == b.shape and (a == b).all(), (label, f)


@functools.lru_cache(maxsize=None)
def check_cases(name: str, n: int = 4):
    """[(label, model before, model after, model pub, expected flag names, expected (array, index, reason) or None)]"""
    cp = pm.CURVES[name]
    G1, G2 = pm.groups(cp)
    sec, before = cc.honest(name, n)
    mine = contribution_secrets(cp)
    after = sc.model_srs(cp, n, contributed(cp, sec, mine))
    pub = model_pub(cp, sec, mine)
    out = [("honest", before, after, pub, set(), None)]
    other = tuple((s * 5 + 3) % cp.r for s in mine)
    opub = model_pub(cp, sec, other)
    assert all(o != p for o, p in zip(opub, pub))
    for k, flag in enumerate((TAU_RATIO, ALPHA_RATIO, BETA_RATIO)):
        p = list(pub)
        p[k] = opub[k]
        out.append(("pub.%s of another secret" % PUB_FIELDS[k], before, after, p, {flag}, None))
    out.append(("pub alpha / beta swapped", before, after, [pub[0], pub[2], pub[1]], {ALPHA_RATIO, BETA_RATIO}, None))
    # `after` descends from an SRS of other secrets with the same generators: well formed, the generators agree, every ratio is off
    sec2 = dict(sec, tau=(sec["tau"] + 1) % cp.r, alpha=(sec["alpha"] + 1) % cp.r, beta=(sec["beta"] + 1) % cp.r)
    after2 = sc.model_srs(cp, n, contributed(cp, sec2, mine))
    assert after2["tau_g1"][0] == before["tau_g1"][0] and after2["tau_g2"][0] == before["tau_g2"][0]
    out.append(("after of a different before", before, after2, pub, {TAU_RATIO, ALPHA_RATIO, BETA_RATIO}, None))
    # another pair of generators, everything else honest: each array of `after` is still a sequence of powers, and the ratios hold
    # against the OLD g2 only if the G1 generator is the old one
    sec3 = dict(sec, g1=G1.mul(sec["g1"], 2))
    after3 = sc.model_srs(cp, n, contributed(cp, sec3, mine))
    out.append(("g1 generator changed", before, after3, pub, {SHAPE, TAU_RATIO, ALPHA_RATIO, BETA_RATIO}, None))
    _, longer = cc.honest(name, n, 1)
    assert len(longer["tau_g1"]) == len(before["tau_g1"]) + 1 and longer["tau_g1"][:2] == before["tau_g1"][:2]
    out.append(("lengths differ", longer, after, pub, {SHAPE}, None))
    # one tampered point of `after`: what ceremony_cases predicts for that SRS on its own (its honest SRS is `before`, so the cases
    # are rebuilt on `after` by the same tampering)
    dbl = lambda P: G1.add(P, P)  # noqa: E731
    a = {k: list(v) for k, v in after.items()}
    a["tau_g1"][2] = dbl(after["tau_g1"][2])
    out.append(("after.tau_g1[2] doubled", before, a, pub, {cc.TAU_G1}, None))
    a = {k: list(v) for k, v in after.items()}
    a["beta_tau_g1"][n - 1] = dbl(after["beta_tau_g1"][n - 1])
    out.append(("after.beta_tau_g1[last] doubled", before, a, pub, {cc.BETA}, None))
    a = {k: list(v) for k, v in after.items()}
    a["tau_g2"][n - 1] = None
    out.append(("after.tau_g2[last] identity", before, a, pub, {cc.BAD_POINT}, ("tau_g2", n - 1, cc.IDENTITY)))
    # bad points of the record and of `before`
    p = list(pub)
    p[1] = cc.off_curve_point(G2, pub[1])
    out.append(("pub.alpha_g2 off curve", before, after, p, {cc.BAD_POINT}, ("pub_alpha_g2", 0, cc.OFF_CURVE)))
    p = list(pub)
    p[2] = None
    out.append(("pub.beta_g2 identity", before, after, p, {cc.BAD_POINT}, ("pub_beta_g2", 0, cc.IDENTITY)))
    Q = cc.outside_subgroup_point(name, True)
    if Q is not None:
        p = list(pub)
        p[0] = Q
        out.append(("pub.tau_g2 outside subgroup", before, after, p, {cc.BAD_POINT}, ("pub_tau_g2", 0, cc.OFF_SUBGROUP)))
    b = {k: list(v) for k, v in before.items()}
    b["alpha_tau_g1"][0] = cc.off_curve_point(G1, before["alpha_tau_g1"][0])
    out.append(("before.alpha_tau_g1[0] off curve", b, after, pub, {cc.BAD_POINT}, ("before", 3, cc.OFF_CURVE)))
    return out
