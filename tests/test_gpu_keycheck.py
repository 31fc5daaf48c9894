"""GPU tier: the key check without the derivation on the MI355X.  fold_key_from_srs against its host twin, byte for byte (the twin is
held against the big-integer model by test_keycheck_host.py), from the one-point domain to 2^12 points, both curves and both
reductions; check_key_derivation on keys made by generate_parameters_from_srs + contribute_delta, every tamper of keycheck_cases.py,
the verdict against check_parameters' derivation-based one; check_parameters(derive=False); coefficients.  No tolerance anywhere."""
import numpy as np
import pytest

import ceremony_cases as cc
import keycheck_cases as kc
import pymodel as pm
import srs_cases as sc
from helpers import arr_to_g1, g1_to_arr

pytestmark = pytest.mark.gpu
QAPS = [sc.LIBSNARK, sc.CIRCOM]
QAP_IDS = ["libsnark", "circom"]
SRS_FIELDS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module")
def provers(g):
    made = {}

    def get(cp, qap=sc.LIBSNARK):
        if (cp.name, qap) not in made:
            made[(cp.name, qap)] = g.Groth16(cp.name, 0, qap=g.LibsnarkReduction if qap == sc.LIBSNARK else g.CircomReduction)
        return made[(cp.name, qap)]

    yield get
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def gens(orc):
    """a non-standard pair of generators per curve (the oracle's setup draws one)"""
    return {cp.name: orc.setup(orc.syn_circuit(cp.name, 2, 1), 3)[1] for cp in sc.CURVES}


@pytest.fixture(scope="module")
def srs_of(orc, provers, gens):
    """the SRS of a domain of n points per curve, made on the GPU once: (srs, the SRS of another tau)"""
    made = {}

    def get(cp, n):
        if (cp.name, n) not in made:
            tau, alpha, beta, tau2 = orc.rand_fr(cp.name, 91, 4)
            g1, g2 = gens[cp.name]["g1gen"], gens[cp.name]["g2gen"]
            made[(cp.name, n)] = (provers(cp).srs_from_trapdoor(n, tau, alpha, beta, g1, g2), provers(cp).srs_from_trapdoor(n, tau2, alpha, beta, g1, g2))
        return made[(cp.name, n)]

    return get


def _qap(g, qap):
    return g.LibsnarkReduction if qap == sc.LIBSNARK else g.CircomReduction


def _half_padded(cp, k):
    """num_constraints + num_inputs = 2^k + 1: a domain of 2^(k+1) points, half of it padding rows"""
    cs = pm.syn_circuit(cp, k, 3)[0]
    cs.a.append([(1, 1), (5, 0)])
    cs.b.append([(1, 0)])
    cs.c.append([(1, 1), (5, 0)])
    assert cs.num_constraints + cs.num_inputs == (1 << k) + 1
    return cs


def _big_circuits(cp):
    yield "syn8", pm.syn_circuit(cp, 8, 3, dense=True)[0]
    yield "half_padded_2^8", _half_padded(cp, 7)
    yield "syn12", pm.syn_circuit(cp, 12, 5)[0]


# ---- values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_fold_equals_host_twin_small(g, provers, cp, qap):
    """the circuits of the CPU tier: domains of 1, 4, 8 and 16 points, empty rows, a variable in no row, no l_query"""
    prover = provers(cp, qap)
    for name, cs in kc.host_circuits(cp):
        n = sc.domain_size(cs)
        mats = kc.mats_of(g, cp, cs)
        srs = sc.srs_to_arrays(g, cp, cc.honest(cp.name, n)[1])
        co = kc.coeffs_for(cs, qap)
        kc.assert_fold_equal(prover.fold_key_from_srs(mats, srs, co), g.fold_key_from_srs_host(cp.name, mats, srs, co, _qap(g, qap)), name)


@pytest.mark.parametrize("name", ["syn8", "half_padded_2^8", "syn12"])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_fold_equals_host_twin(g, provers, srs_of, cp, qap, name):
    """2^8 and 2^12 points: more than one block of the row kernel, several passes of the transforms, Circom's 2n-point transform one
    size above the n-point ones, a domain whose upper half is padding"""
    prover = provers(cp, qap)
    cs = dict(_big_circuits(cp))[name]
    n = sc.domain_size(cs)
    assert n == (1 << 12 if name == "syn12" else 1 << 8)
    mats = kc.mats_of(g, cp, cs)
    srs, _ = srs_of(cp, n)
    co = kc.coeffs_for(cs, qap)
    got = prover.fold_key_from_srs(mats, srs, co)
    kc.assert_fold_equal(got, g.fold_key_from_srs_host(cp.name, mats, srs, co, _qap(g, qap)), name)
    kc.assert_fold_equal(prover.fold_key_from_srs(mats, srs, co), got, (name, "deterministic"))
    tm = prover.keycheck_timings()
    assert tm["window_bits"] > 0 and tm["windows"] > 0 and tm["rows_ms"] > 0 and tm["passes_ms"] > 0 and tm["membership_ms"] == 0, tm


# ---- verdicts --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys_2_8(g, orc, provers, srs_of):
    made = {}

    def get(cp, qap):
        if (cp.name, qap) not in made:
            prover = provers(cp, qap)
            cs = pm.syn_circuit(cp, 8, 3)[0]
            mats = kc.mats_of(g, cp, cs)
            srs, other = srs_of(cp, 1 << 8)
            d1, d2, d3 = orc.rand_fr(cp.name, 57, 3)
            k0 = prover.generate_parameters_from_srs(mats, srs)
            k1 = prover.contribute_delta(k0, d1)
            k3 = prover.contribute_delta(prover.contribute_delta(k1, d2), d3)
            cs2 = pm.R1CS(cs.num_inputs, cs.num_witness, [list(r) for r in cs.a], cs.b, cs.c)
            cf, col = cs2.a[100][0]
            cs2.a[100][0] = ((cf + 1) % cp.r, col)
            made[(cp.name, qap)] = dict(cs=cs, mats=mats, srs=srs, other_srs=other, k0=k0, k1=k1, k3=k3,
                                        other_tau=prover.generate_parameters_from_srs(mats, other),
                                        other_a=prover.generate_parameters_from_srs(kc.mats_of(g, cp, cs2), srs))
        return made[(cp.name, qap)]

    return get


@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_check_key_derivation_flags(g, provers, keys_2_8, cp, qap):
    prover = provers(cp, qap)
    k = keys_2_8(cp, qap)
    mats, srs = k["mats"], k["srs"]
    co = kc.coeffs_for(k["cs"], qap, 29)
    for label in ("k0", "k1", "k3"):
        cc.assert_result(prover.check_key_derivation(mats, srs, k[label], co), set(), None, ("honest", label))
    tm = prover.keycheck_timings()
    assert tm["membership_ms"] > 0 and tm["pairings_ms"] > 0 and tm["sorts_ms"] > 0, tm
    cases = kc.tamper_cases(g, cp, k["k3"], k["k0"], k["other_tau"], k["other_a"], mats.num_instance_variables)
    for i, (label, bad, expect, where) in enumerate(cases):
        res = prover.check_key_derivation(mats, srs, bad, co)
        kc.assert_case(res, expect, where, label)
        if label in ("a_query swap", "two bad points"):      # the host twin agrees, named point included (its membership tests are slow)
            host = g.check_key_derivation_host(cp.name, mats, srs, bad, co, _qap(g, qap))
            assert (res.flags, res.array, res.index, res.reason) == (host.flags, host.array, host.index, host.reason), label
    # h_query of the other reduction's length: a shape error, not a flag; a key held on the device only: TypeError
    cut = cc.key_copy(g, k["k3"])
    cut.h_query = cut.h_query[:-1] if qap == sc.CIRCOM else np.concatenate([cut.h_query, cut.h_query[:1]])
    with pytest.raises(ValueError):
        prover.check_key_derivation(mats, srs, cut, co)
    with pytest.raises(TypeError):
        prover.check_key_derivation(mats, srs, g.DeviceProvingKey.__new__(g.DeviceProvingKey), co)


@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_verdict_equals_check_parameters(g, provers, keys_2_8, cp, qap):
    """the verdict is check_parameters' (default derive=True: it derives the key again), on the honest key and on three tampers"""
    prover = provers(cp, qap)
    k = keys_2_8(cp, qap)
    mats, srs = k["mats"], k["srs"]
    co = kc.coeffs_for(k["cs"], qap, 29)
    cases = kc.tamper_cases(g, cp, k["k3"], k["k0"], k["other_tau"], k["other_a"], mats.num_instance_variables)
    srs_co = cc.random_coeffs(2 * (1 << 8) - 2, 3)
    assert bool(prover.check_parameters(mats, srs, k["k3"], srs_co)) and bool(prover.check_key_derivation(mats, srs, k["k3"], co))
    for label in ("a_query[last]", "l_query[0]", "another tau"):
        bad = next(c[1] for c in cases if c[0] == label)
        assert not prover.check_parameters(mats, srs, bad, srs_co) and not prover.check_key_derivation(mats, srs, bad, co), label


@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_check_parameters_without_derivation(g, provers, keys_2_8, cp):
    prover = provers(cp, sc.LIBSNARK)
    k = keys_2_8(cp, sc.LIBSNARK)
    mats, srs = k["mats"], k["srs"]
    co = cc.random_coeffs(2 * (1 << 8) - 2, 7)      # enough for the SRS and for the key
    res = prover.check_parameters(mats, srs, k["k3"], co, derive=False)
    cc.assert_result(res, set(), None, "honest")
    assert prover.check_parameters(mats, srs, k["k1"], derive=False)
    res = prover.check_parameters(mats, srs, k["other_a"], co, derive=False)
    assert "A" in res.failed and not res
    res = prover.check_parameters(mats, k["other_srs"], k["k3"], co, derive=False)      # another honest SRS: the key's equations fail
    assert "A" in res.failed and "H" in res.failed and "BAD_POINT" not in res.failed
    # a broken SRS: the check_srs failure comes back first, although the key is broken too
    bad_srs = g.SRS(srs.curve, **{f: np.ascontiguousarray(getattr(srs, f)).copy() for f in SRS_FIELDS})
    last = len(srs.tau_g1) - 1
    P = arr_to_g1(srs.tau_g1[last:last + 1], cp)[0]
    bad_srs.tau_g1[last] = g1_to_arr([pm.groups(cp)[0].add(P, P)], cp)[0]
    res = prover.check_parameters(mats, bad_srs, k["other_a"], co, derive=False)
    assert res.failed == ("TAU_G1",)


# ---- coefficients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_coefficients(g, provers, keys_2_8, cp):
    prover = provers(cp, sc.CIRCOM)
    k = keys_2_8(cp, sc.CIRCOM)
    mats, srs = k["mats"], k["srs"]
    bad = cc.key_copy(g, k["k3"])
    j = cc.first_nonidentity(bad.l_query, step=-1)
    bad.l_query[j] = cc._scaled_row(cp, bad.l_query, j, 2)
    for _ in range(2):                                # fresh coefficients: the honest key passes and the tampered one fails, every time
        assert prover.check_key_derivation(mats, srs, k["k3"])
        assert prover.check_key_derivation(mats, srs, bad).failed == ("L",)
    n, ni, nv, nh = kc.shape(k["cs"], sc.CIRCOM)
    need = max(nv, nh)
    co = cc.random_coeffs(need, 31)
    with pytest.raises(g.G16Error) as e:
        prover.check_key_derivation(mats, srs, k["k3"], co[:need - 1])
    assert e.value.status == 2 and "coefficients" in str(e.value)
    with pytest.raises(g.G16Error) as e:
        prover.check_key_derivation(mats, srs, k["k3"], co[:need - 1] + [0])
    assert e.value.status == 3
    with pytest.raises(g.G16Error) as e:
        prover.fold_key_from_srs(mats, srs, co[:3] + [0] + co[4:])
    assert e.value.status == 3
    with pytest.raises(ValueError):
        prover.fold_key_from_srs(mats, srs, None)
    short = g.SRS(srs.curve, srs.tau_g1[:-1], srs.tau_g2, srs.alpha_tau_g1, srs.beta_tau_g1, srs.beta_g2)
    with pytest.raises(g.G16Error) as e:
        prover.check_key_derivation(mats, short, k["k3"], co)
    assert e.value.status == 2 and "tau_g1" in str(e.value)
