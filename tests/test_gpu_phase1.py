"""GPU tier of phase 1 on the MI355X: batch_scalar_mul against its host twin (byte for byte: the scalar and point sets of the CPU tier,
wave borders for one lane per G1 point and a lane pair per G2 point, waves full of small-order points and waves with one, out
aliasing points, a chunk that splits a wave); contribute_tau against the model SRS of the multiplied secrets; check_tau_contribution
against its host twin on every case of the CPU tier; the contributed SRS through generate_parameters_from_srs(check=True);
determinism.  No tolerance anywhere."""
import numpy as np
import pytest

import ceremony_cases as cc
import phase1_cases as pc
import pymodel as pm
import srs_cases as sc
import table_cases as tc
from helpers import circuit_from_pymodel, ints_to_mont

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]
G_IDS = ["g1", "g2"]


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module")
def provers(g):
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = g.Groth16(curve, 0)
        return made[curve]

    yield get
    for p in made.values():
        p.close()


def _same(got, want, labels):
    bad = [labels[i] for i in range(len(labels)) if (got[i] != want[i]).any()]
    assert not bad, (len(bad), bad[:8])


# ---- the unit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g2", [False, True], ids=G_IDS)
@pytest.mark.parametrize("curve", CURVES)
def test_batch_scalar_mul_equals_host_twin(g, provers, curve, g2):
    """every case of the CPU tier in one call (several waves), then the sizes around a wave: one lane per G1 point, a pair per G2 point"""
    prover = provers(curve)
    cases = pc.smul_cases(curve, g2)
    pts, ks, _ = pc.smul_arrays(curve, g2, cases)
    want = g.batch_scalar_mul_host(curve, pts, ks)
    labels = [c[0] for c in cases]
    _same(prover.batch_scalar_mul(pts, ks), want, labels)
    tm = prover.phase1_timings()
    assert tm["mul_g2_ms" if g2 else "mul_g1_ms"] > 0 and tm["mul_g1_ms" if g2 else "mul_g2_ms"] == 0 and tm["powers_ms"] == 0, tm
    for n in ((1, 31, 32, 33, 65) if g2 else (1, 63, 64, 65, 129)):
        idx = [(5 + 7 * i) % len(cases) for i in range(n)]   # strides through the scalar list and the special points alike
        _same(prover.batch_scalar_mul(pts[idx], ks[idx]), want[idx], [labels[i] for i in idx])
    assert prover.batch_scalar_mul(pts[:0], ks[:0]).shape == pts[:0].shape   # n = 0: a no-op


@pytest.mark.parametrize("g2", [False, True], ids=G_IDS)
@pytest.mark.parametrize("curve", CURVES)
def test_small_order_points_fill_a_wave_or_sit_alone(g, provers, curve, g2):
    """equal or opposite operands inside the window walk: the slow path taken by every lane of a wave, by exactly one, and by none"""
    prover = provers(curve)
    m = tc.model(curve, g2)
    cp = pm.CURVES[curve]
    T = tc.tasks_per_wave(g2)
    small = pc.small_order_points(curve, g2)
    mult = dict(tc.point_classes(curve, g2))["multiple of the generator"]
    kvals = [k for _, k in pc.scalars(curve)]
    ks_int = [kvals[(3 * i + 1) % len(kvals)] for i in range(T)]
    ks = np.ascontiguousarray(ints_to_mont(ks_int, cp.r, 4))
    full = [small[i % len(small)] for i in range(T)]
    lone = [mult[i % len(mult)] for i in range(T)]
    lone[17] = small[1]
    none = [mult[i % len(mult)] for i in range(T)]
    for label, points in (("every lane", full), ("one lane", lone), ("no lane", none)):
        pts = np.array([tc.abi_words(m, P) for P in points], dtype=np.uint64)
        got = prover.batch_scalar_mul(pts, ks)
        assert (got == g.batch_scalar_mul_host(curve, pts, ks)).all(), label
        model = np.array([tc.abi_words(m, pc.expected(curve, g2, P, k)) for P, k in zip(points, ks_int)], dtype=np.uint64)
        assert (got == model).all(), label


@pytest.mark.parametrize("g2", [False, True], ids=G_IDS)
@pytest.mark.parametrize("curve", CURVES)
def test_out_may_alias_points_and_a_chunk_may_split_a_wave(g, provers, curve, g2, monkeypatch):
    from groth16_amd.binding import ptr64

    prover = provers(curve)
    cases = pc.smul_cases(curve, g2)[100:229]
    pts, ks, _ = pc.smul_arrays(curve, g2, cases)
    want = g.batch_scalar_mul_host(curve, pts, ks)
    buf = pts.copy()
    lb = g.lib()
    lb.check(lb.ph1.g16_batch_scalar_mul(prover._ctx.handle, int(g2), ptr64(buf.reshape(-1)), ptr64(ks.reshape(-1)), len(buf), ptr64(buf.reshape(-1))))
    assert (buf == want).all()
    monkeypatch.setenv("G16_PHASE1_CHUNK", "37")   # 129 points: launches of 37, 37, 37 and 18
    assert (prover.batch_scalar_mul(pts, ks) == want).all()


# ---- a contribution --------------------------------------------------------------------------------------------------------------
def _model_contribution(g, cp, n, extra):
    sec, before = cc.honest(cp.name, n, extra)
    mine = pc.contribution_secrets(cp, 77 + n)
    want = sc.model_srs(cp, n, pc.contributed(cp, sec, mine), extra)
    return sec, mine, sc.srs_to_arrays(g, cp, before), sc.srs_to_arrays(g, cp, want)


@pytest.mark.parametrize("n,extra", [(4, 0), (16, 3), (64, 0)])
@pytest.mark.parametrize("curve", CURVES)
def test_contribute_tau_equals_model(g, provers, curve, n, extra, monkeypatch):
    """n = 64: the 126 tau_g1 points go through the powers kernel in runs of 16 (eight lanes), and once more one per lane in launches of
    100 and 26 points: the first spans two waves of the powers kernel and ends inside the second wave of the multiplication"""
    cp = pm.CURVES[curve]
    prover = provers(curve)
    sec, mine, before, want = _model_contribution(g, cp, n, extra)
    assert len(before.tau_g1) == 2 * n - 1 + extra and len(before.tau_g2) == n + extra
    secrets = [sc.fr(cp, s) for s in mine]
    wp = pc.pub_to_arrays(g, cp, pc.model_pub(cp, sec, mine))
    for env in ({}, {"G16_PHASE1_CHUNK": "100", "G16_PHASE1_RUN": "1"}) if n == 64 else ({},):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        after, pub = prover.contribute_tau(before, *secrets)
        pc.assert_srs_equal(after, want, (n, env))
        assert (after.tau_g1[0] == before.tau_g1[0]).all() and (after.tau_g2[0] == before.tau_g2[0]).all()   # the generators, bit for bit
        for f in pc.PUB_FIELDS:
            assert (getattr(pub, f) == getattr(wp, f)).all(), f
        tm = prover.phase1_timings()
        assert tm["powers_ms"] > 0 and tm["mul_g1_ms"] > 0 and tm["mul_g2_ms"] > 0, tm
    if n == 4:
        with pytest.raises(g.UnexpectedIdentity):
            prover.contribute_tau(before, secrets[0], sc.fr(cp, 0), secrets[2])
        hafter, hpub = g.contribute_tau_host(curve, before, *secrets)
        pc.assert_srs_equal(after, hafter, "host twin")


# ---- the check ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_check_tau_contribution_equals_host_twin(g, provers, curve):
    cp = pm.CURVES[curve]
    prover = provers(curve)
    n = 4
    coeffs = cc.random_coeffs(2 * n)
    for label, before, after, pub, expect, where in pc.check_cases(curve, n):
        args = (sc.srs_to_arrays(g, cp, before), sc.srs_to_arrays(g, cp, after), pc.pub_to_arrays(g, cp, pub), coeffs)
        res = prover.check_tau_contribution(*args)
        cc.assert_result(res, expect, where, label)
        assert res == g.check_tau_contribution_host(curve, *args), label
        assert res == prover.check_tau_contribution(*args), label   # explicit coefficients: the call is deterministic


@pytest.mark.parametrize("curve", CURVES)
def test_contributed_srs_passes_the_checks_and_yields_a_key(g, provers, curve):
    cp = pm.CURVES[curve]
    prover = provers(curve)
    n = 4
    before = sc.srs_to_arrays(g, cp, cc.honest(curve, n)[1])
    after, pub = prover.contribute_tau(before)   # secrets from the operating system
    assert prover.check_tau_contribution(before, after, pub).ok
    assert not prover.check_tau_contribution(after, before, pub)
    name, cs, z = next(sc.host_circuits(cp))
    assert sc.domain_size(cs) == n
    mats = sc.mats_of(g, circuit_from_pymodel(cp, cs, z))
    key = prover.generate_parameters_from_srs(mats, after, check=True)
    sc.assert_keys_equal(key, g.generate_parameters_from_srs_host(curve, mats, after), "key from the contributed SRS")
