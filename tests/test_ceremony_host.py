"""CPU tier: the ceremony checks through their host twins (g16_host_rlc_sums, g16_host_srs_check, g16_host_params_check_delta) -- plain
scalar multiplications, the host membership tests and the host pairing -- against the big-int model's MSM and against the flag sets
that ceremony_cases.py derives in the exponent.  Keys come from srs_cases.trapdoor_key: the key in the exponent with gamma = 1 and
any delta, which the setup tests hold byte-equal to generate_parameters_from_srs + contribute_delta."""
import numpy as np
import pytest

import ceremony_cases as cc
import pymodel as pm
import srs_cases as sc
from helpers import g1_to_arr, g2_to_arr


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


def _points(cp, g2, n, seed):
    """n subgroup points; an identity and a P, -P pair among them when there is room"""
    G = pm.groups(cp)[1 if g2 else 0]
    gen = cp.g2 if g2 else cp.g1
    rng = pm.SplitMix64(seed)
    ks = [rng.field(cp.r - 1) + 1 for _ in range(n)]
    if n >= 4:
        ks[1], ks[3] = 0, (-ks[2]) % cp.r
    return [G.mul(gen, k) if k else None for k in ks]


@pytest.mark.parametrize("n", [1, 2, 3, 9])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_host_rlc_sums_match_model_msm(g, cp, g2, n):
    G = pm.groups(cp)[1 if g2 else 0]
    conv = g2_to_arr if g2 else g1_to_arr
    pts = _points(cp, g2, n, 31 + n)
    arr = conv(pts, cp)
    for label, co in cc.coeff_edge_cases(max(n - 1, 1)).items():
        co = co[:n - 1]
        lo, hi = g.rlc_sums_host(cp.name, arr, cc.coeff_array(co))
        mlo, mhi = cc.model_sums(G, pts, co)
        assert (lo == conv([mlo], cp)[0]).all() and (hi == conv([mhi], cp)[0]).all(), (label, n)
        if n == 1:
            assert not lo.any() and not hi.any()
    # Python integers and (n, 2) word arrays are the same coefficients; None draws fresh ones
    co = cc.random_coeffs(max(n - 1, 1))[:n - 1]
    a, b = g.rlc_sums_host(cp.name, arr, co), g.rlc_sums_host(cp.name, arr, cc.coeff_array(co))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    g.rlc_sums_host(cp.name, arr, None)


@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_host_srs_check_flags(g, cp):
    coeffs = cc.random_coeffs(6)   # N1 = 7, N2 = M = 4: one vector of max - 1 = 6 serves every array
    for label, srs, expect, where in cc.srs_cases(cp.name, 4):
        res = g.check_srs_host(cp.name, sc.srs_to_arrays(g, cp, srs), coeffs)
        cc.assert_result(res, expect, where, label)
    _, srs = cc.honest(cp.name, 4)
    assert g.check_srs_host(cp.name, sc.srs_to_arrays(g, cp, srs))          # coeffs=None: fresh coefficients
    for label, co in cc.coeff_edge_cases(6).items():
        assert g.check_srs_host(cp.name, sc.srs_to_arrays(g, cp, srs), co), label


_KEYS = {}


def _keys(g, cp, name, cs, qap):
    """delta = 1, delta_1 and delta_1 delta_2 keys of one circuit, in the exponent"""
    k = (cp.name, name, qap)
    if k not in _KEYS:
        sec = sc.secrets(cp)
        d1, d2 = sec["delta"], (sec["delta"] * 7 + 3) % cp.r
        _KEYS[k] = [cc.key_from_model(g, cp, sc.trapdoor_key(cp, cs, sec, qap, d)) for d in (1, d1, d1 * d2 % cp.r)]
    return _KEYS[k]


@pytest.mark.parametrize("qap", [sc.LIBSNARK, sc.CIRCOM], ids=["libsnark", "circom"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_host_delta_check_flags(g, cp, qap):
    for name, cs, z in sc.host_circuits(cp):
        if name == "syn4":
            continue
        k0, k1, k2 = _keys(g, cp, name, cs, qap)
        coeffs = cc.random_coeffs(max(len(k0.l_query), len(k0.h_query)), 11)
        # honest: one and two chained contributions, against the predecessor and against the delta = 1 key
        for before, after in ((k0, k1), (k1, k2), (k0, k2), (k0, k0)):
            res = g.check_delta_contribution_host(cp.name, before, after, coeffs)
            cc.assert_result(res, set(), None, (name, "honest"))
        assert g.check_delta_contribution_host(cp.name, k0, k2)   # coeffs=None
        for label, bad, expect, where in cc.key_tamper_cases(g, cp, k2):
            for before in (k1, k0):
                res = g.check_delta_contribution_host(cp.name, before, bad, coeffs)
                cc.assert_result(res, expect, where, (name, label))


def test_host_refusals(g):
    cp = pm.BN254
    _, srs = cc.honest(cp.name, 4)
    arr = sc.srs_to_arrays(g, cp, srs)
    fields = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
    for field, keep in (("tau_g1", 1), ("tau_g2", 1), ("alpha_tau_g1", 0)):
        short = g.SRS(cp.name, **{f: (getattr(arr, f)[:keep] if f == field else getattr(arr, f)) for f in fields})
        with pytest.raises(g.G16Error) as e:
            g.check_srs_host(cp.name, short)
        assert e.value.status == 2 and field in str(e.value), (field, str(e.value))
    with pytest.raises(g.G16Error) as e:            # N1 = 7 needs 6 coefficients
        g.check_srs_host(cp.name, arr, cc.random_coeffs(5))
    assert e.value.status == 2 and "coefficients" in str(e.value)
    co = cc.random_coeffs(6)
    co[5] = 0                                       # the one coefficient only the last tau_g1 point meets
    with pytest.raises(g.G16Error) as e:
        g.check_srs_host(cp.name, arr, co)
    assert e.value.status == 3
    with pytest.raises(g.G16Error) as e:
        g.rlc_sums_host(cp.name, arr.tau_g1, [1, 0, 3, 4, 5, 6])
    assert e.value.status == 3
    with pytest.raises(ValueError):
        g.rlc_sums_host(cp.name, arr.tau_g1, [1, 2])
    with pytest.raises(ValueError):
        g.check_srs_host("bls12_381", arr)          # an SRS of the other curve
    with pytest.raises(ValueError):
        g.rlc_sums_host(cp.name, arr.tau_g1, [1 << 128] * 6)
    # keys: shapes must agree, explicit coefficients must cover l_query and h_query
    name, cs, z = next(sc.host_circuits(cp))
    k0, k1, _ = _keys(g, cp, name, cs, sc.LIBSNARK)
    cut = cc.key_copy(g, k1)
    cut.l_query = cut.l_query[:-1]
    with pytest.raises(ValueError):
        g.check_delta_contribution_host(cp.name, k0, cut)
    with pytest.raises(ValueError):
        g.check_delta_contribution_host("bls12_381", k0, k1)
    need = max(len(k0.l_query), len(k0.h_query))
    with pytest.raises(g.G16Error) as e:
        g.check_delta_contribution_host(cp.name, k0, k1, cc.random_coeffs(need - 1))
    assert e.value.status == 2
    with pytest.raises(g.G16Error) as e:
        g.check_delta_contribution_host(cp.name, k0, k1, [0] * need)
    assert e.value.status == 3


def test_result_object(g):
    cp = pm.BN254
    cases = {label: (srs, expect, where) for label, srs, expect, where in cc.srs_cases(cp.name, 4)}
    srs, expect, where = cases["two bad points"]
    res = g.check_srs_host(cp.name, sc.srs_to_arrays(g, cp, srs), cc.random_coeffs(6))
    assert not res and not res.ok and res.flags == 1 and res.failed == ("BAD_POINT",) and (res.array, res.index, res.reason) == where
    err = g.BadSRS(res)
    assert err.result is res and "tau_g2[3]" in str(err)
    ok = g.check_srs_host(cp.name, sc.srs_to_arrays(g, cp, cc.honest(cp.name, 4)[1]), cc.random_coeffs(6))
    assert ok and ok.ok and ok.flags == 0 and ok.failed == () and ok.array is None and ok.index is None
