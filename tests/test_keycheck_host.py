"""CPU tier of the key check without the derivation (libg16_keycheck.so, no GPU): the host twins against the big-integer model.

Values: fold_key_from_srs_host -- a row walk over the matrices, scalar transforms and MSMs over the SRS -- must give, bit for bit,
sum_j rho_j (key point j) over the key that generate_parameters_from_srs_host DERIVES with group transforms; the sum is made here
with pymodel's group arithmetic.  Verdicts: honest keys after 0, 1 and 3 delta contributions pass, every tamper of
keycheck_cases.py raises exactly its flag.  Domains stay at 16 points or below: the model is slow."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ceremony_cases as cc
import keycheck_cases as kc
import pymodel as pm
import srs_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QAPS = [sc.LIBSNARK, sc.CIRCOM]
QAP_IDS = ["libsnark", "circom"]


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


def _qap(g, qap):
    return g.LibsnarkReduction if qap == sc.LIBSNARK else g.CircomReduction


def _srs(g, cp, n, sec=None):
    if sec is None:
        return sc.srs_to_arrays(g, cp, cc.honest(cp.name, n)[1])
    return sc.srs_to_arrays(g, cp, sc.model_srs(cp, n, sec))


# ---- values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_fold_equals_sums_over_the_derived_key(g, cp, qap):
    for name, cs in kc.host_circuits(cp):
        n, ni, nv, nh = kc.shape(cs, qap)
        mats = kc.mats_of(g, cp, cs)
        srs = _srs(g, cp, n)
        key = g.generate_parameters_from_srs_host(cp.name, mats, srs, _qap(g, qap))
        assert len(key.h_query) == nh and len(key.l_query) == nv - ni
        if name == "sparse":
            assert not key.a_query[6].any() and not key.b_g2_query[6].any() and not key.l_query[6 - ni].any()   # a variable in no row
        co = kc.coeffs_for(cs, qap)
        got = g.fold_key_from_srs_host(cp.name, mats, srs, co, _qap(g, qap))
        assert set(got) == set(kc.FOLD_POINTS)
        kc.assert_fold_equal(got, kc.model_fold(cp, key, ni, co), (name, "model"))
        # more coefficients than needed: the prefix is used; integers and word arrays are the same coefficients
        again = g.fold_key_from_srs_host(cp.name, mats, srs, cc.coeff_array(co + [5, 7]), _qap(g, qap))
        kc.assert_fold_equal(again, got, (name, "prefix"))
        if nv == ni:
            assert not got["l"].any()
        if nh == 0:
            assert not got["h"].any()


def test_fold_refusals(g):
    cp = pm.BN254
    cs = pm.syn_circuit(cp, 2, 3)[0]
    mats, srs = kc.mats_of(g, cp, cs), _srs(g, cp, 4)
    co = kc.coeffs_for(cs, sc.CIRCOM)
    with pytest.raises(ValueError):
        g.fold_key_from_srs_host(cp.name, mats, srs, None)
    with pytest.raises(g.G16Error) as e:                     # Circom: h_query has n = 4 points, the variables are 5
        g.fold_key_from_srs_host(cp.name, mats, srs, co[:4], g.CircomReduction)
    assert e.value.status == 2 and "coefficients" in str(e.value)
    with pytest.raises(g.G16Error) as e:
        g.fold_key_from_srs_host(cp.name, mats, srs, co[:2] + [0] + co[3:])
    assert e.value.status == 3
    short = g.SRS(cp.name, srs.tau_g1[:6], srs.tau_g2, srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2)
    with pytest.raises(g.G16Error) as e:
        g.fold_key_from_srs_host(cp.name, mats, short, co)
    assert e.value.status == 2 and "tau_g1" in str(e.value)
    bad = g.ConstraintMatrices(mats.num_instance_variables, mats.num_witness_variables, mats.num_constraints,
                               (mats.a[0], np.full_like(np.asarray(mats.a[1]), 5), mats.a[2]), mats.b, mats.c)
    with pytest.raises(g.G16Error) as e:                     # column 5 of 5 variables: refused before any gather
        g.fold_key_from_srs_host(cp.name, bad, srs, co)
    assert e.value.status == 2 and "column" in str(e.value)
    with pytest.raises(ValueError):
        g.fold_key_from_srs_host("bls12_381", mats, srs, co)


# ---- verdicts --------------------------------------------------------------------------------------------------------------------
def _keys(g, cp, cs, qap, sec):
    """the key in the exponent (gamma = 1) after 0, 1 and 3 delta contributions"""
    d = [sec["delta"], (sec["delta"] * 7 + 3) % cp.r, (sec["delta"] * 11 + 5) % cp.r]
    return [cc.key_from_model(g, cp, sc.trapdoor_key(cp, cs, sec, qap, x)) for x in (1, d[0], d[0] * d[1] * d[2] % cp.r)]


@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_honest_keys_pass(g, cp, qap):
    sec = sc.secrets(cp)
    for name, cs in kc.host_circuits(cp):
        n, ni, nv, nh = kc.shape(cs, qap)
        mats, srs = kc.mats_of(g, cp, cs), _srs(g, cp, n)
        co = kc.coeffs_for(cs, qap, 23)
        derived = g.generate_parameters_from_srs_host(cp.name, mats, srs, _qap(g, qap))
        for label, key in zip(("derived", "delta = 1", "one contribution", "three contributions"), [derived] + _keys(g, cp, cs, qap, sec)):
            res = g.check_key_derivation_host(cp.name, mats, srs, key, co, _qap(g, qap))
            cc.assert_result(res, set(), None, (name, label))
    assert g.check_key_derivation_host(cp.name, mats, srs, derived, None, _qap(g, qap))      # fresh coefficients


@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_tampered_keys_raise_their_flag(g, cp, qap):
    sec = sc.secrets(cp)
    cs = pm.syn_circuit(cp, 3, 4)[0]
    n, ni, nv, nh = kc.shape(cs, qap)
    mats, srs = kc.mats_of(g, cp, cs), _srs(g, cp, n)
    k0, k1, k3 = _keys(g, cp, cs, qap, sec)
    sec2 = dict(sec, tau=(sec["tau"] * 3 + 1) % cp.r)
    other_tau = cc.key_from_model(g, cp, sc.trapdoor_key(cp, cs, sec2, qap, 1))
    cs2 = pm.R1CS(cs.num_inputs, cs.num_witness, [list(r) for r in cs.a], cs.b, cs.c)
    cf, col = cs2.a[1][0]
    cs2.a[1][0] = ((cf + 1) % cp.r, col)
    other_a = g.generate_parameters_from_srs_host(cp.name, kc.mats_of(g, cp, cs2), srs, _qap(g, qap))
    co = kc.coeffs_for(cs, qap, 29)
    for label, bad, expect, where in kc.tamper_cases(g, cp, k3, k0, other_tau, other_a, ni):
        res = g.check_key_derivation_host(cp.name, mats, srs, bad, co, _qap(g, qap))
        kc.assert_case(res, expect, where, label)
    res = g.check_key_derivation_host(cp.name, mats, srs, kc.tamper_cases(g, cp, k1, k0, other_tau, other_a, ni)[0][1], None, _qap(g, qap))
    assert res.failed == ("A",)                                                            # fresh coefficients find it too
    # h_query of the other reduction's length: a shape error, not a flag
    cut = cc.key_copy(g, k3)
    cut.h_query = cut.h_query[:-1] if qap == sc.CIRCOM else np.concatenate([cut.h_query, cut.h_query[:1]])
    with pytest.raises(ValueError):
        g.check_key_derivation_host(cp.name, mats, srs, cut, co, _qap(g, qap))
    with pytest.raises(g.G16Error) as e:
        g.check_key_derivation_host(cp.name, mats, srs, k3, co[:max(nv, nh) - 1], _qap(g, qap))
    assert e.value.status == 2
    with pytest.raises(g.G16Error) as e:
        g.check_key_derivation_host(cp.name, mats, srs, k3, [0] * max(nv, nh), _qap(g, qap))
    assert e.value.status == 3


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_library_loads_and_header_matches_exports(g):
    from groth16_amd import binding

    kcl = g.lib().kc
    for name in binding.KEYCHECK_EXPORTS:
        assert hasattr(kcl, name), name
    hdr = open(os.path.join(ROOT, "include", "g16_keycheck.h")).read()
    assert set(re.findall(r"\b(g16_[a-z0-9_]+)\s*\(", hdr)) == set(binding.KEYCHECK_EXPORTS)
    for name in ("check_key_derivation", "fold_key_from_srs", "keycheck_timings"):
        assert hasattr(g.Groth16, name), name
    for name in ("check_key_derivation_host", "fold_key_from_srs_host"):
        assert name in g.__all__ and hasattr(g, name)
    # the flag table of the header is the one the Python side decodes with
    from groth16_amd import groth16 as mod

    flags = {name: int(v) for name, v in re.findall(r"#define G16_KEYCHECK_([A-Z0-9_]+) (\d+)u", hdr)}
    assert flags == {v: k for k, v in mod.KEY_DERIVATION_FLAGS.items()}


def test_header_compiles_as_strict_c99():
    src = '#include "g16_keycheck.h"\nint main(void) { g16_keycheck_timings t; g16_key_fold f; (void)t; (void)f; return (int)G16_KEYCHECK_H - 256; }\n'
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "consumer.c")
        with open(path, "w") as f:
            f.write(src)
        out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), path],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
