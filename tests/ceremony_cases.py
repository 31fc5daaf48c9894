"""Ceremony checks: the cases the CPU and GPU tiers share (TEST INFRASTRUCTURE), built on srs_cases.py and subgroup_cases.py.

Every case starts from an honest SRS (or key) made from known secrets with non-standard generators and tampers with it in the
model, where every point's discrete logarithm is known, so the expected flag set follows in the exponent.  With g1, g2 the
generators, L = sum rho_i X[i] ("lo") and H = sum rho_i X[i + 1] ("hi") of an array X, and t2 = the exponent of tau_g2[1]:

  TAU_G1   t2 * lo(tau_g1)  == hi(tau_g1)            ALPHA / BETA   the same over alpha_tau_g1 / beta_tau_g1
  TAU_G2   log(tau_g1[1]) * lo(tau_g2) == log(tau_g1[0]) * hi(tau_g2)
  BETA_G2  log(beta_tau_g1[0]) == log(tau_g1[0]) * log(beta_g2)

Two expectations differ from the issue that asked for these tests, because the equations it fixes say otherwise:
  * tau_g1[1] replaced: the issue lists {TAU_G1}, but TAU_G2 reads tau_g1[1] as its G1 point, so the set is {TAU_G1, TAU_G2}; the
    pure {TAU_G1} case is shown at index 2 as well as at the middle and last index.
  * tau_g2 built from tau' != tau: the issue lists {TAU_G1, TAU_G2}, but ALPHA and BETA compare against tau_g2[1] = tau' g2 too
    (tau' lo(alpha) != tau lo(alpha) = hi(alpha)), so the set is {TAU_G1, TAU_G2, ALPHA, BETA}.
The generators assert their premises (a tampered point differs from the honest one, lies where it should) with the big-int model."""
import functools

import numpy as np

import pymodel as pm
import srs_cases as sc
import subgroup_cases as sg
from helpers import arr_to_g1, arr_to_g2, g1_to_arr, g2_to_arr

BAD_POINT, TAU_G1, TAU_G2, ALPHA, BETA, BETA_G2 = "BAD_POINT", "TAU_G1", "TAU_G2", "ALPHA", "BETA", "BETA_G2"
FIXED_PART, DELTA, L, H = "FIXED_PART", "DELTA", "L", "H"
SRS_ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
SRS_G2 = ("tau_g2", "beta_g2")
OFF_CURVE, OFF_SUBGROUP, IDENTITY = 2, 3, 4
KEY_FIXED_NAMES = ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query")
MASK64 = (1 << 64) - 1


def coeff_array(vals) -> np.ndarray:
    return np.array([[v & MASK64, v >> 64] for v in vals], dtype=np.uint64).reshape(-1, 2)


def random_coeffs(m: int, seed: int = 0xC0FFEE):
    rng = pm.SplitMix64(seed)
    out = []
    while len(out) < m:
        v = rng.next() | (rng.next() << 64)
        if v:
            out.append(v)
    return out


def digit_coeff(c: int) -> int:
    """a 128-bit rho whose every c-bit window holds 2^(c-1): the value the signed-digit bias turns into a carry in every window"""
    v, w = 0, 0
    while w * c + c - 1 < 128:
        v |= 1 << (w * c + c - 1)
        w += 1
    assert 0 < v < 1 << 128 and all((v >> (k * c)) & ((1 << c) - 1) == 1 << (c - 1) for k in range(w))
    return v


def coeff_edge_cases(m: int, c_values=(4, 5, 7, 8, 11, 13, 16)):
    """{label: m coefficients}; the all-windows case for every window size a plan may pick for small inputs (the GPU tier adds the
    size the plan reports)"""
    out = {"all_max": [(1 << 128) - 1] * m, "all_one": [1] * m, "top_bit": [1 << 127] * m, "random": random_coeffs(m)}
    for c in c_values:
        out[f"windows_c{c}"] = [digit_coeff(c)] * m
    mixed = random_coeffs(m, 7)
    for k in range(m):
        if k % 3 == 0:
            mixed[k] = (1 << 128) - 1 - k
        elif k % 3 == 1:
            mixed[k] = 1 << (127 - k % 64)
    out["mixed"] = mixed
    return out


def model_sums(G, pts, coeffs):
    """(lo, hi) by the model's MSM over the two shifted slices"""
    m = len(pts) - 1
    return (G.msm(pts[:m], coeffs[:m]) if m else None), (G.msm(pts[1:], coeffs[:m]) if m else None)


# ---- SRS cases -------------------------------------------------------------------------------------------------------------
def _copy(srs):
    return {k: list(v) for k, v in srs.items()}


def off_curve_point(G, P):
    Q = (P[0], G.F.add(P[1], G.F.one))
    assert not G.on_curve(Q)
    return Q


@functools.lru_cache(maxsize=None)
def outside_subgroup_point(name: str, g2: bool):
    """a point of the curve outside the prime-order subgroup (None where the cofactor is 1)"""
    if sg.cofactor(name, g2) == 1:
        return None
    flagged, _ = sg.cases(name, g2)
    P = next(P for label, P, f in flagged if label.startswith("member+order") and f == 0)
    return P


@functools.lru_cache(maxsize=None)
def honest(name: str, n: int, extra: int = 0):
    cp = pm.CURVES[name]
    sec = sc.secrets(cp)
    return sec, sc.model_srs(cp, n, sec, extra)


def srs_cases(name: str, n: int, bad_points: bool = True):
    """[(label, model SRS, expected flag names, expected (array, index, reason) or None)] for a domain of n points"""
    cp = pm.CURVES[name]
    G1, G2 = pm.groups(cp)
    sec, srs = honest(name, n)
    p = cp.r
    N1, M = len(srs["tau_g1"]), len(srs["alpha_tau_g1"])
    assert N1 == 2 * n - 1 and M == n and len(srs["tau_g2"]) == n and N1 >= 5
    out = [("honest", srs, set(), None)]

    def tamper(label, field, idx, point, expect):
        s = _copy(srs)
        assert point != s[field][idx] and point is not None and (G2 if field in SRS_G2 else G1).on_curve(point), label
        s[field][idx] = point
        out.append((label, s, set(expect), None))

    dbl = lambda G, P: G.add(P, P)  # noqa: E731
    # one tau_g1 point replaced by its double (a subgroup point): rho_(i-1) in hi and rho_i in lo see it, the last one only in hi
    tamper("tau_g1[1] doubled", "tau_g1", 1, dbl(G1, srs["tau_g1"][1]), {TAU_G1, TAU_G2})   # TAU_G2's G1 point is tau_g1[1]
    tamper("tau_g1[2] doubled", "tau_g1", 2, dbl(G1, srs["tau_g1"][2]), {TAU_G1})
    tamper("tau_g1[mid] doubled", "tau_g1", N1 // 2, dbl(G1, srs["tau_g1"][N1 // 2]), {TAU_G1})
    tamper("tau_g1[last] doubled", "tau_g1", N1 - 1, dbl(G1, srs["tau_g1"][N1 - 1]), {TAU_G1})
    # g1 itself: lo(tau_g1) moves, TAU_G2 and BETA_G2 read g1; alpha / beta do not
    tamper("tau_g1[0] doubled", "tau_g1", 0, dbl(G1, srs["tau_g1"][0]), {TAU_G1, TAU_G2, BETA_G2})
    s = _copy(srs)
    k = N1 // 2
    assert k >= 2 and s["tau_g1"][k] != s["tau_g1"][k + 1]
    s["tau_g1"][k], s["tau_g1"][k + 1] = s["tau_g1"][k + 1], s["tau_g1"][k]
    out.append(("tau_g1 adjacent swap", s, {TAU_G1}, None))
    # tau_g2[i] = tau'^i g2.  TAU_G2: tau S vs tau' S for S = sum rho_i tau'^i != 0.  TAU_G1, ALPHA, BETA: tau' lo vs hi = tau lo.
    tau2 = (sec["tau"] * 3 + 1) % p
    assert tau2 not in (sec["tau"], 0, 1)
    s = _copy(srs)
    s["tau_g2"] = [G2.mul(sec["g2"], pow(tau2, i, p)) for i in range(len(srs["tau_g2"]))]
    assert s["tau_g2"][0] == srs["tau_g2"][0] and s["tau_g2"][1] != srs["tau_g2"][1]
    out.append(("tau_g2 from tau'", s, {TAU_G1, TAU_G2, ALPHA, BETA}, None))
    # alpha_tau_g1[i] = alpha tau'^i g1: entry 0 (= alpha_g1 of a key) is untouched, no other equation reads the array
    s = _copy(srs)
    s["alpha_tau_g1"] = [G1.mul(sec["g1"], sec["alpha"] * pow(tau2, i, p) % p) for i in range(M)]
    assert s["alpha_tau_g1"][0] == srs["alpha_tau_g1"][0]
    out.append(("alpha from tau'", s, {ALPHA}, None))
    beta2 = (sec["beta"] + 5) % p
    tamper("beta_g2 from beta'", "beta_g2", 0, G2.mul(sec["g2"], beta2), {BETA_G2})
    tamper("beta_tau_g1[last] doubled", "beta_tau_g1", M - 1, dbl(G1, srs["beta_tau_g1"][M - 1]), {BETA})
    if not bad_points:
        return out
    # bad points: the identity, a point off the curve, a curve point outside the subgroup -- in every array
    for a, field in enumerate(SRS_ARRAYS):
        g2 = field in SRS_G2
        G = G2 if g2 else G1
        idx = len(srs[field]) - 1 if field != "tau_g1" else 3
        kinds = [("identity", None, IDENTITY), ("off curve", off_curve_point(G, srs[field][idx]), OFF_CURVE)]
        Q = outside_subgroup_point(name, g2)
        if Q is not None:
            assert G.on_curve(Q)
            kinds.append(("outside subgroup", Q, OFF_SUBGROUP))
        for kind, point, reason in kinds:
            s = _copy(srs)
            s[field][idx] = point
            out.append((f"{field}[{idx}] {kind}", s, {BAD_POINT}, (field, idx, reason)))
    # two bad points in different arrays: the first in field order is reported, whatever the indices
    s = _copy(srs)
    s["beta_tau_g1"][0] = None
    s["tau_g2"][len(srs["tau_g2"]) - 1] = off_curve_point(G2, srs["tau_g2"][-1])
    out.append(("two bad points", s, {BAD_POINT}, ("tau_g2", len(srs["tau_g2"]) - 1, OFF_CURVE)))
    s = _copy(srs)
    s["tau_g1"][4], s["tau_g1"][2] = None, off_curve_point(G1, srs["tau_g1"][2])
    out.append(("two bad points in one array", s, {BAD_POINT}, ("tau_g1", 2, OFF_CURVE)))
    return out


# ---- key cases -------------------------------------------------------------------------------------------------------------
def key_copy(g, pk):
    cp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64).copy()  # noqa: E731
    return g.ProvingKey(pk.curve, *[cp(getattr(pk, f)) for f in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "b_g1_query",
                                                                 "b_g2_query", "h_query", "l_query", "gamma_g2", "gamma_abc_g1")])


def key_from_model(g, cp, key) -> "object":
    a = sc.key_to_arrays(cp, key)
    return g.ProvingKey(cp.name, a["alpha_g1"], a["beta_g1"], a["delta_g1"], a["beta_g2"], a["delta_g2"], a["a_query"], a["b_g1_query"],
                        a["b_g2_query"], a["h_query"], a["l_query"], a["gamma_g2"], a["gamma_abc_g1"])


def _scaled_row(cp, arr, idx, k, g2=False):
    """row idx of a point array multiplied by k in the model"""
    G = pm.groups(cp)[1 if g2 else 0]
    P = (arr_to_g2 if g2 else arr_to_g1)(arr[idx:idx + 1], cp)[0]
    assert P is not None
    Q = G.mul(P, k)
    assert Q != P and Q is not None
    return (g2_to_arr if g2 else g1_to_arr)([Q], cp)[0]


def first_nonidentity(arr, start=0, step=1):
    idx = range(start, len(arr), step) if step > 0 else range(len(arr) - 1, -1, -1)
    for i in idx:
        if arr[i].any():
            return i
    raise AssertionError("every point of the array is the identity")


def key_tamper_cases(g, cp, after):
    """[(label, tampered copy of `after`, expected flag names, expected (array, index) or None)]: `after` is an honest successor of
    the key it will be checked against"""
    out = []

    def case(label, expect, where=None):
        k = key_copy(g, after)
        out.append((label, k, set(expect), where))
        return k

    nl, nh = len(after.l_query), len(after.h_query)
    assert nl >= 2 and nh >= 2
    i0, i1 = first_nonidentity(after.l_query), first_nonidentity(after.l_query, step=-1)
    k = case("l_query first doubled", {L})
    k.l_query[i0] = _scaled_row(cp, after.l_query, i0, 2)
    k = case("l_query last doubled", {L})
    k.l_query[i1] = _scaled_row(cp, after.l_query, i1, 2)
    assert i0 != i1 and (after.l_query[i0] != after.l_query[i1]).any()
    k = case("l_query swap", {L})
    k.l_query[[i0, i1]] = after.l_query[[i1, i0]]
    j = first_nonidentity(after.h_query, nh // 2)
    k = case("h_query one point", {H})
    k.h_query[j] = _scaled_row(cp, after.h_query, j, 3)
    # delta_1 alone: the ratio of the G1 deltas no longer matches that of the G2 deltas; l and h are judged against delta_2
    k = case("delta_g1 alone", {DELTA})
    k.delta_g1[0] = _scaled_row(cp, after.delta_g1, 0, 5)
    # delta_2 from another delta: every equation reads it
    k = case("delta_g2 from another delta", {DELTA, L, H})
    k.delta_g2[0] = _scaled_row(cp, after.delta_g2, 0, 7, g2=True)
    # l and h scaled by different deltas: one of them no longer matches the deltas
    k = case("h scaled by another delta", {H})
    for i in range(nh):
        if after.h_query[i].any():
            k.h_query[i] = _scaled_row(cp, after.h_query, i, 11)
    k = case("l scaled by another delta", {L})
    for i in range(nl):
        if after.l_query[i].any():
            k.l_query[i] = _scaled_row(cp, after.l_query, i, 11)
    ja = first_nonidentity(after.a_query, len(after.a_query) // 2)
    k = case("a_query changed", {FIXED_PART}, ("a_query", ja))
    k.a_query[ja] = _scaled_row(cp, after.a_query, ja, 2)
    jb = first_nonidentity(after.b_g2_query, step=-1)
    k = case("b_g2_query changed", {FIXED_PART}, ("b_g2_query", jb))
    k.b_g2_query[jb] = _scaled_row(cp, after.b_g2_query, jb, 2, g2=True)
    jg = first_nonidentity(after.gamma_abc_g1)
    k = case("gamma_abc_g1 changed", {FIXED_PART}, ("gamma_abc_g1", jg))
    k.gamma_abc_g1[jg] = _scaled_row(cp, after.gamma_abc_g1, jg, 2)
    # bad points of the moving part: the deltas may not be the identity, l / h may
    k = case("delta_g1 identity", {BAD_POINT}, ("delta_g1", 0, IDENTITY))
    k.delta_g1[0] = 0
    k = case("l_query off curve", {BAD_POINT}, ("l_query", i1, OFF_CURVE))
    k.l_query[i1] = g1_to_arr([off_curve_point(pm.groups(cp)[0], arr_to_g1(after.l_query[i1:i1 + 1], cp)[0])], cp)[0]
    return out


def assert_result(res, expect, where, label):
    assert set(res.failed) == set(expect), (label, res.failed, expect)
    assert bool(res) == (not expect) and res.ok == (not expect), label
    if where is not None:
        assert (res.array, res.index) == tuple(where[:2]), (label, res.array, res.index, where)
        if len(where) > 2:
            assert res.reason == where[2], (label, res.reason, where)
