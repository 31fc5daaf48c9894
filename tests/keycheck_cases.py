"""The key check without the derivation: circuits, the model's sums and the tampers the CPU and GPU tiers share (TEST
INFRASTRUCTURE), built on srs_cases.py, ceremony_cases.py and subgroup_cases.py.

The value tests hold fold_key_from_srs against  sum_j rho_j (key point j)  over a DERIVED key, summed with pymodel's group
arithmetic: the identity the whole check rests on, shown on values and not just on verdicts.  The tampers are made on arrays, on a
copy of an honest key; every replacement is a subgroup point (the double of the original, or another point of the key where the
original is the identity), so each must raise its own flag and never BAD_POINT."""
import numpy as np

import ceremony_cases as cc
import pymodel as pm
import srs_cases as sc
from helpers import arr_to_g1, arr_to_g2, circuit_from_pymodel, g1_to_arr, g2_to_arr

A, B_G1, B_G2, GAMMA_ABC, L, H, FIXED, DELTA, BAD_POINT = "A", "B_G1", "B_G2", "GAMMA_ABC", "L", "H", "FIXED", "DELTA", "BAD_POINT"
FOLD_POINTS = ("a", "b_g1", "b_g2", "gamma_abc", "l", "h")


def sparse_circuit(cp, seed: int = 9):
    """2 instance and 5 witness variables, 5 rows: coefficients that are not one, terms of instance variables in A, B and C (the
    `in` sums), a column named twice in one row, empty rows of A and of B, and variable 6 in no row at all (its query points are the
    identity)"""
    rng = pm.SplitMix64(seed)
    f = lambda: rng.field(cp.r - 2) + 2  # noqa: E731
    a = [[(f(), 0), (1, 2), (f(), 3)], [], [(1, 1), (f(), 1), (f(), 4)], [(f(), 5)], [(1, 2)]]
    b = [[(1, 3)], [(f(), 2), (f(), 0)], [], [(f(), 1), (1, 4)], [(f(), 5), (f(), 5)]]
    c = [[(f(), 4)], [(1, 0)], [(f(), 5), (1, 1)], [], [(f(), 3), (f(), 2)]]
    return pm.R1CS(2, 5, a, b, c)


def host_circuits(cp):
    """(name, R1CS) for the CPU tier: domains of 1 to 16 points"""
    yield "syn2", pm.syn_circuit(cp, 2, 3)[0]
    yield "syn3", pm.syn_circuit(cp, 3, 4)[0]
    cs = pm.mimc_circuit(cp, 5, 2)[0]
    assert sc.domain_size(cs) != cs.num_constraints + cs.num_inputs     # a padded domain
    yield "mimc5", cs
    yield "sparse", sparse_circuit(cp)
    rng = pm.SplitMix64(5)
    f = lambda: rng.field(cp.r - 2) + 2  # noqa: E731
    yield "all_inputs", pm.R1CS(3, 0, [[(f(), 0), (1, 1)], [(f(), 2)]], [[(1, 2)], [(f(), 1), (f(), 0)]], [[(f(), 1)], [(1, 0), (f(), 2)]])   # no l_query
    yield "one_point", pm.R1CS(1, 0, [], [], [])                       # a one-point domain: no constraint, the constant-one wire alone


def mats_of(g, cp, cs):
    return sc.mats_of(g, circuit_from_pymodel(cp, cs, [0] * (cs.num_inputs + cs.num_witness)))


def shape(cs, qap):
    n = sc.domain_size(cs)
    return n, cs.num_inputs, cs.num_inputs + cs.num_witness, (n if qap == sc.CIRCOM else n - 1)


def coeffs_for(cs, qap, seed=17):
    n, ni, nv, nh = shape(cs, qap)
    co = cc.random_coeffs(max(nv, nh), seed)
    co[0] = (1 << 128) - 1                   # the largest coefficient on the constant-one wire
    return co


def _msm(G, pts, co):
    live = [(P, k) for P, k in zip(pts, co) if P is not None]
    return G.msm([P for P, _ in live], [k for _, k in live]) if live else None


def model_fold(cp, key, ni: int, co):
    """sum_j rho_j (key point j) per equation over a key given as arrays, in pymodel's group arithmetic; the points as arrays"""
    G1, G2 = pm.groups(cp)
    g1 = lambda arr: arr_to_g1(arr, cp)  # noqa: E731
    nv = len(key.a_query)
    out = dict(a=_msm(G1, g1(key.a_query), co[:nv]), b_g1=_msm(G1, g1(key.b_g1_query), co[:nv]),
               b_g2=_msm(G2, arr_to_g2(key.b_g2_query, cp), co[:nv]), gamma_abc=_msm(G1, g1(key.gamma_abc_g1), co[:ni]),
               l=_msm(G1, g1(key.l_query), co[ni:nv]), h=_msm(G1, g1(key.h_query), co))
    return {k: (g2_to_arr if k == "b_g2" else g1_to_arr)([v], cp)[0] for k, v in out.items()}


def assert_fold_equal(got, want, label):
    for k in FOLD_POINTS:
        assert (np.asarray(got[k]).reshape(-1) == np.asarray(want[k]).reshape(-1)).all(), (label, k)


# ---- tampers ---------------------------------------------------------------------------------------------------------------------
def _changed(cp, arr, idx, g2=False):
    """a subgroup point that differs from arr[idx]: its double, or -- where it is the identity -- another point of the array"""
    if arr[idx].any():
        return cc._scaled_row(cp, arr, idx, 2, g2)
    j = cc.first_nonidentity(arr)
    return arr[j].copy()


def tamper_cases(g, cp, honest, delta1_key, other_tau_key, other_a_key, ni: int):
    """[(label, key, expected flags or a predicate on the failed set, expected (array, index[, reason]) or None)].
    honest: the key under test (any delta); delta1_key: the delta = 1 key of the same circuit and SRS; other_tau_key: the same circuit
    over an SRS with another tau (the same generators, alpha, beta); other_a_key: the same SRS, one coefficient of A changed"""
    out = []

    def case(label, expect, where=None, base=None):
        k = cc.key_copy(g, base if base is not None else honest)
        out.append((label, k, expect, where))
        return k

    nv, nl, nh = len(honest.a_query), len(honest.l_query), len(honest.h_query)
    assert ni >= 2 and nl >= 2 and nh >= 2
    for label, idx in (("a_query[0] (the constant-one wire)", 0), ("a_query at an instance index", ni - 1), ("a_query[last]", nv - 1)):
        k = case(label, {A})
        k.a_query[idx] = _changed(cp, honest.a_query, idx)
    i0, i1 = cc.first_nonidentity(honest.a_query), cc.first_nonidentity(honest.a_query, step=-1)
    assert i0 != i1 and (honest.a_query[i0] != honest.a_query[i1]).any()
    k = case("a_query swap", {A})
    k.a_query[[i0, i1]] = honest.a_query[[i1, i0]]
    jb = cc.first_nonidentity(honest.b_g1_query, nv // 2)
    k = case("b_g1_query changed", {B_G1})
    k.b_g1_query[jb] = _changed(cp, honest.b_g1_query, jb)
    k = case("b_g2_query changed", {B_G2})
    k.b_g2_query[jb] = _changed(cp, honest.b_g2_query, jb, g2=True)
    k = case("b_g2_query from another key", {B_G2})
    assert (other_tau_key.b_g2_query != honest.b_g2_query).any()
    k.b_g2_query[:] = other_tau_key.b_g2_query
    k = case("gamma_abc_g1 changed", {GAMMA_ABC})
    k.gamma_abc_g1[ni - 1] = _changed(cp, honest.gamma_abc_g1, ni - 1)
    for label, idx in (("l_query[0]", 0), ("l_query[last]", nl - 1)):
        k = case(label, {L})
        k.l_query[idx] = _changed(cp, honest.l_query, idx)
    for label, idx in (("h_query[0]", 0), ("h_query[last]", nh - 1)):
        k = case(label, {H})
        k.h_query[idx] = _changed(cp, honest.h_query, idx)
    if (honest.delta_g1 != delta1_key.delta_g1).any():
        k = case("l and h left at delta = 1", {L, H})
        k.l_query[:] = delta1_key.l_query
        k.h_query[:] = delta1_key.h_query
    k = case("delta_g1 of another delta", {DELTA})
    k.delta_g1[0] = cc._scaled_row(cp, honest.delta_g1, 0, 5)
    k = case("alpha_g1 replaced", {FIXED}, ("alpha_g1", 0))
    k.alpha_g1[0] = cc._scaled_row(cp, honest.alpha_g1, 0, 3)
    case("one coefficient of A changed", lambda failed: A in failed and BAD_POINT not in failed, base=other_a_key)
    case("another tau", lambda failed: A in failed and BAD_POINT not in failed, base=other_tau_key)
    # bad points: exclusive, the first array in the order of the header, its smallest index
    G1 = pm.groups(cp)[0]
    jl = cc.first_nonidentity(honest.l_query, step=-1)
    k = case("l_query off curve", {BAD_POINT}, ("l_query", jl, cc.OFF_CURVE))
    k.l_query[jl] = g1_to_arr([cc.off_curve_point(G1, arr_to_g1(honest.l_query[jl:jl + 1], cp)[0])], cp)[0]
    k = case("two bad points", {BAD_POINT}, ("b_g1_query", 1, cc.OFF_CURVE))
    for idx in (nv - 1, 1):
        P = arr_to_g1(honest.a_query[i0:i0 + 1], cp)[0]
        k.b_g1_query[idx] = g1_to_arr([cc.off_curve_point(G1, P)], cp)[0]
    k.h_query[0] = k.b_g1_query[1]
    k = case("delta_g2 the identity", {BAD_POINT}, ("delta_g2", 0, cc.IDENTITY))
    k.delta_g2[0] = 0
    for g2, field in ((False, "a_query"), (True, "b_g2_query")):
        Q = cc.outside_subgroup_point(cp.name, g2)
        if Q is not None:        # BLS12-381 (both groups); BN254's G1 has cofactor 1
            k = case(f"{field} outside the subgroup", {BAD_POINT}, (field, 2, cc.OFF_SUBGROUP))
            getattr(k, field)[2] = (g2_to_arr if g2 else g1_to_arr)([Q], cp)[0]
    return out


def assert_case(res, expect, where, label):
    if callable(expect):
        assert expect(set(res.failed)) and not res, (label, res.failed)
        return
    cc.assert_result(res, expect, where, label)
