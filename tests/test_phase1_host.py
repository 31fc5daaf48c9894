"""CPU tier of phase 1 (libg16_phase1.so, no GPU): the host twins against the big-integer models.

batch_scalar_mul_host runs plain double-and-add; windowed=True runs the DEVICE kernel's task (signed 4-bit window, lazy 30-bit
arithmetic, selections instead of branches, the slow path for equal / opposite operands) lane by lane on the host, so the
algorithm the GPU runs is held against the model here, before any GPU sees it.  Every comparison is exact."""
import numpy as np
import pytest

import ceremony_cases as cc
import phase1_cases as pc
import pymodel as pm
import srs_cases as sc

CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


def test_exports(g):
    from groth16_amd import binding

    ph1 = g.lib().ph1
    for name in binding.PHASE1_EXPORTS:
        assert hasattr(ph1, name), name
    for name in ("TauContribution", "batch_scalar_mul_host", "contribute_tau_host", "check_tau_contribution_host"):
        assert hasattr(g, name) and name in g.__all__, name
    for name in ("batch_scalar_mul", "contribute_tau", "check_tau_contribution", "phase1_timings"):
        assert hasattr(g.Groth16, name), name


@pytest.mark.parametrize("curve", CURVES)
def test_reference_recoding(curve):
    for label, k in pc.scalars(curve):
        d = pc.recode(k)
        assert len(d) == 64 and sum(x * 16 ** j for j, x in enumerate(d)) == k, label
    labels = [label for label, _ in pc.scalars(curve)]
    assert "2^4" in labels and "2^4-1" in labels and "2^248" in labels and "2^252-1" in labels


@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "windowed"])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("curve", CURVES)
def test_batch_scalar_mul_host(g, curve, g2, windowed):
    cases = pc.smul_cases(curve, g2)
    pts, ks, want = pc.smul_arrays(curve, g2, cases)
    got = g.batch_scalar_mul_host(curve, pts, ks, windowed=windowed)
    bad = [cases[i][0] for i in range(len(cases)) if (got[i] != want[i]).any()]
    assert not bad, (len(bad), bad[:8])
    # every scalar on the subgroup points: the same values from pymodel's own group (its mul, with its reduction modulo r)
    if not windowed:
        cp = pm.CURVES[curve]
        G = pm.groups(cp)[1 if g2 else 0]
        for label, P, k in cases[:len(pc.scalars(curve))]:
            assert pc.expected(curve, g2, P, k) == (G.mul(P, k) if P is not None and k else None), label


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("curve", CURVES)
def test_batch_scalar_mul_host_edges(g, curve, g2):
    cases = pc.smul_cases(curve, g2)[:5]
    pts, ks, want = pc.smul_arrays(curve, g2, cases)
    assert g.batch_scalar_mul_host(curve, pts[:0], ks[:0]).shape == pts[:0].shape   # n = 0: a no-op
    with pytest.raises(ValueError):
        g.batch_scalar_mul_host(curve, pts, ks[:3])
    # out aliasing points, straight through the C ABI
    from groth16_amd.binding import CURVE_ID, ptr64

    lb = g.lib()
    buf = pts.copy()
    lb.check(lb.ph1.g16_host_batch_scalar_mul(CURVE_ID[curve], int(g2), ptr64(buf.reshape(-1)), ptr64(ks.reshape(-1)), len(buf), ptr64(buf.reshape(-1))))
    assert (buf == want).all()


def _contribution(g, cp, n, extra=0, mine=None):
    sec, before = cc.honest(cp.name, n, extra)
    mine = mine or pc.contribution_secrets(cp)
    want = sc.model_srs(cp, n, pc.contributed(cp, sec, mine), extra)
    return sec, mine, sc.srs_to_arrays(g, cp, before), sc.srs_to_arrays(g, cp, want)


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("curve", CURVES)
def test_contribute_tau_host(g, curve, n):
    cp = pm.CURVES[curve]
    sec, mine, before, want = _contribution(g, cp, n)
    keep = sc.srs_to_arrays(g, cp, cc.honest(curve, n)[1])
    after, pub = g.contribute_tau_host(curve, before, *[sc.fr(cp, s) for s in mine])
    pc.assert_srs_equal(after, want, "contributed")
    pc.assert_srs_equal(before, keep, "the input SRS is untouched")
    wp = pc.pub_to_arrays(g, cp, pc.model_pub(cp, sec, mine))
    for f in pc.PUB_FIELDS:
        assert (getattr(pub, f) == getattr(wp, f)).all(), f


@pytest.mark.parametrize("curve", CURVES)
def test_contribute_tau_host_special_secrets(g, curve):
    cp = pm.CURVES[curve]
    n = 4
    G1 = pm.groups(cp)[0]
    sec, before_m = cc.honest(curve, n)
    before = sc.srs_to_arrays(g, cp, before_m)
    one = sc.fr(cp, 1)
    # tau' = 1 leaves the tau arrays byte-identical (alpha' = beta' = 1: the whole SRS)
    after, _ = g.contribute_tau_host(curve, before, one, one, one)
    pc.assert_srs_equal(after, before, "unit contribution")
    # tau' = r - 1 negates the odd indices
    after, _ = g.contribute_tau_host(curve, before, sc.fr(cp, cp.r - 1), one, one)
    from helpers import g1_to_arr

    want = g1_to_arr([P if i % 2 == 0 else G1.neg(P) for i, P in enumerate(before_m["tau_g1"])], cp)
    assert (after.tau_g1 == want).all() and (after.tau_g1[0] == before.tau_g1[0]).all() and (after.tau_g2[0] == before.tau_g2[0]).all()
    # two contributions compose
    m1, m2 = pc.contribution_secrets(cp, 5), pc.contribution_secrets(cp, 6)
    a1, _ = g.contribute_tau_host(curve, before, *[sc.fr(cp, s) for s in m1])
    a2, _ = g.contribute_tau_host(curve, a1, *[sc.fr(cp, s) for s in m2])
    both = tuple(x * y % cp.r for x, y in zip(m1, m2))
    pc.assert_srs_equal(a2, sc.srs_to_arrays(g, cp, sc.model_srs(cp, n, pc.contributed(cp, sec, both))), "two contributions")
    # a zero secret is refused and nothing is written
    from groth16_amd.binding import CURVE_ID, ptr64

    lb = g.lib()
    for k in range(3):
        s = [sc.fr(cp, 3), sc.fr(cp, 4), sc.fr(cp, 5)]
        s[k] = sc.fr(cp, 0)
        with pytest.raises(g.UnexpectedIdentity):
            g.contribute_tau_host(curve, before, *s)
        work = sc.srs_to_arrays(g, cp, before_m)
        pub = pc.pub_to_arrays(g, cp, [None] * 3)
        sv, keep = work.view()
        pv, pkeep = pub.view()
        import ctypes as C

        rc = lb.ph1.g16_host_srs_contribute(CURVE_ID[curve], ptr64(s[0]), ptr64(s[1]), ptr64(s[2]), C.byref(sv), C.byref(pv), None)
        assert rc == 8
        pc.assert_srs_equal(work, before, "refused: nothing written")
        assert not any(a.any() for a in pkeep)


@pytest.mark.parametrize("curve", CURVES)
def test_check_tau_contribution_host(g, curve):
    cp = pm.CURVES[curve]
    n = 4
    coeffs = cc.random_coeffs(2 * n)
    for label, before, after, pub, expect, where in pc.check_cases(curve, n):
        res = g.check_tau_contribution_host(curve, sc.srs_to_arrays(g, cp, before), sc.srs_to_arrays(g, cp, after), pc.pub_to_arrays(g, cp, pub),
                                            coeffs)
        cc.assert_result(res, expect, where, label)
        if where is None:
            assert res.array is None and res.index is None and res.reason == 0, label


@pytest.mark.parametrize("curve", CURVES)
def test_contribution_round_trip_host(g, curve):
    """contribute, then check what came out: the two halves agree with each other, not only with the model"""
    cp = pm.CURVES[curve]
    before = sc.srs_to_arrays(g, cp, cc.honest(curve, 4)[1])
    after, pub = g.contribute_tau_host(curve, before)   # secrets from the operating system
    res = g.check_tau_contribution_host(curve, before, after, pub)
    assert res.ok and res.failed == (), res
    assert (after.tau_g1[1] != before.tau_g1[1]).any()
    assert not g.check_tau_contribution_host(curve, after, before, pub)
