"""CPU tier: the Lagrange form of an SRS through the host twins of libg16_lagrange.so -- the device kernels' own tasks (the butterfly's
sum and difference, the windowed twiddle multiplication) run on the host -- against the host twins of the existing path
(g16_host_group_ntt, g16_host_generate_parameters_srs) and against the big-int model.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest

import lagrange_cases as lc
import pymodel as pm
import srs_cases as sc
from helpers import arr_to_g1, arr_to_g2, g1_to_arr, g2_to_arr, ints_to_mont

QAPS = [sc.LIBSNARK, sc.CIRCOM]
QAP_IDS = ["libsnark", "circom"]
GROUPS = pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
CURVES = pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


def _red(g, qap):
    return g.LibsnarkReduction if qap == sc.LIBSNARK else g.CircomReduction


# ---- the transform ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(7))
@GROUPS
@CURVES
def test_windowed_transform_equals_the_existing_one(g, orc, cp, g2, log_n):
    """random subgroup points with identities, a point next to its negative and a repeated point among them; both directions"""
    n = 1 << log_n
    pts = orc.synth_bases(cp.name, g2, 300 + log_n, n)
    if n >= 8:
        pts[1::4] = 0
        P = (arr_to_g2 if g2 else arr_to_g1)(pts[2:3], cp)[0]
        pts[3] = (g2_to_arr if g2 else g1_to_arr)([pm.groups(cp)[1 if g2 else 0].neg(P)], cp)[0]
        pts[n - 1] = pts[n - 2]
    for inverse in (False, True):
        got = g.group_ntt_windowed_host(cp.name, pts, inverse=inverse)
        assert (got == g.group_ntt_host(cp.name, pts, inverse=inverse)).all(), inverse


@pytest.mark.parametrize("log_n", [0, 1, 2, 3])
@GROUPS
@CURVES
def test_windowed_transform_is_the_dft_sum(g, cp, g2, log_n):
    G = pm.groups(cp)[1 if g2 else 0]
    conv = g2_to_arr if g2 else g1_to_arr
    rng = pm.SplitMix64(11 + log_n)
    n = 1 << log_n
    pts = [G.mul(cp.g2 if g2 else cp.g1, rng.field(cp.r)) for _ in range(n)]
    if n >= 4:
        pts[1], pts[3] = None, G.neg(pts[2])
    arr = conv(pts, cp)
    dom = pm.Domain(cp, n)
    assert (g.group_ntt_windowed_host(cp.name, arr, inverse=False) == conv(sc.model_group_dft(G, pts, dom.omega, cp.r), cp)).all()
    assert (g.group_ntt_windowed_host(cp.name, arr, inverse=True) == conv(sc.model_group_dft(G, pts, dom.omega_inv, cp.r, dom.n_inv), cp)).all()


@pytest.mark.parametrize("log_n", lc.LOG_NS)
@GROUPS
@CURVES
def test_edge_inputs(g, cp, g2, log_n):
    """the edge inputs of lagrange_cases.py: against the existing transform at both sizes, against the model's stages at the small one"""
    for label, pts in lc.edge_inputs(cp.name, g2, log_n):
        arr = lc.to_array(cp.name, g2, pts)
        for inverse in (False, True):
            got = g.group_ntt_windowed_host(cp.name, arr, inverse=inverse)
            assert (got == g.group_ntt_host(cp.name, arr, inverse=inverse)).all(), (label, inverse)
            if log_n == lc.LOG_NS[0]:
                assert (got == lc.to_array(cp.name, g2, lc.model_transform(cp.name, g2, pts, inverse))).all(), (label, inverse, "model")


# ---- the Lagrange form and the key from it -------------------------------------------------------------------------------------------
_CASES = {}


def _case(g, cp, name):
    """(SRS arrays, matrices) of a host circuit, made once per curve; the SRS is two points longer than the domain needs"""
    if (cp.name, name) not in _CASES:
        for nm, cs, z in sc.host_circuits(cp):
            srs = sc.model_srs(cp, sc.domain_size(cs), sc.secrets(cp), extra=2)
            _CASES[(cp.name, nm)] = (sc.srs_to_arrays(g, cp, srs), sc.mats_of(g, sc.flat(cp, cs, z)), sc.domain_size(cs))
    return _CASES[(cp.name, name)]


_KEYS = {}


def _srs_key(g, cp, qap, name, mats, srs):
    """the existing path's key, derived once per case and left unchanged"""
    if (cp.name, qap, name) not in _KEYS:
        _KEYS[(cp.name, qap, name)] = g.generate_parameters_from_srs_host(cp.name, mats, srs, _red(g, qap))
    return _KEYS[(cp.name, qap, name)]


@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@CURVES
def test_prepared_arrays_and_h_basis(g, cp, qap):
    srs, mats, n = _case(g, cp, "syn4")
    lag = g.prepare_srs_host(cp.name, srs, matrices=mats, qap=_red(g, qap))
    assert (lag.log_n, lag.qap, 1 << lag.log_n) == (4, qap, n)
    for name, src in (("u_g1", srs.tau_g1), ("alpha_u_g1", srs.alpha_tau_g1), ("beta_u_g1", srs.beta_tau_g1), ("u_g2", srs.tau_g2)):
        assert (getattr(lag, name) == g.group_ntt_host(cp.name, np.ascontiguousarray(src[:n]), inverse=True)).all(), name
    key = _srs_key(g, cp, qap, "syn4", mats, srs)
    assert lag.h_g1.shape == key.h_query.shape and (lag.h_g1 == key.h_query).all()
    for name, src in (("tau_g1_0", srs.tau_g1), ("alpha_g1_0", srs.alpha_tau_g1), ("beta_g1_0", srs.beta_tau_g1), ("tau_g2_0", srs.tau_g2),
                      ("beta_g2", srs.beta_g2)):
        assert (getattr(lag, name).reshape(-1) == src[0].reshape(-1)).all(), name
    by_log = g.prepare_srs_host(cp.name, srs, log_n=4, qap=_red(g, qap))
    for name in ("u_g1", "alpha_u_g1", "beta_u_g1", "u_g2", "h_g1"):
        assert (getattr(by_log, name) == getattr(lag, name)).all(), name


@pytest.mark.parametrize("name", ["syn2", "syn4", "mimc5"])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@CURVES
def test_key_from_lagrange_equals_key_from_srs(g, cp, qap, name):
    srs, mats, n = _case(g, cp, name)
    lag = g.prepare_srs_host(cp.name, srs, matrices=mats, qap=_red(g, qap))
    got = g.generate_parameters_from_lagrange_host(cp.name, mats, lag, qap=_red(g, qap))
    sc.assert_keys_equal(got, _srs_key(g, cp, qap, name, mats, srs), name)


def _fast_srs(g, cp, n, sec):
    """sc.model_srs through the library's host scalar multiplication: the long crafted circuits need a domain of 256 points"""
    p = cp.r
    pw = [pow(sec["tau"], i, p) for i in range(2 * n - 1)]
    mul = lambda conv, gen, ks: g.batch_scalar_mul_host(cp.name, np.repeat(conv([gen], cp), len(ks), axis=0), ints_to_mont(ks, p, 4))  # noqa: E731
    return g.SRS(cp.name, mul(g1_to_arr, sec["g1"], pw), mul(g2_to_arr, sec["g2"], pw[:n]), mul(g1_to_arr, sec["g1"], [sec["alpha"] * s % p for s in pw[:n]]),
                 mul(g1_to_arr, sec["g1"], [sec["beta"] * s % p for s in pw[:n]]), mul(g2_to_arr, sec["g2"], [sec["beta"]]))


@pytest.mark.parametrize("which", ["coefficients", "one_input", "no_witness", "long_ones", "long_mixed"])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@CURVES
def test_crafted_matrices(g, cp, qap, which):
    """the crafted matrices of the existing path's GPU tests: an empty column, coefficients 0, 1 and r - 1, a constant-one column
    longer than four segments of the sparse product"""
    import test_gpu_srs as tgs

    mats = tgs._crafted(g, cp, which)
    n = 1
    while n < mats.num_constraints + mats.num_instance_variables:
        n <<= 1
    if ("srs", cp.name, n) not in _CASES:
        _CASES[("srs", cp.name, n)] = _fast_srs(g, cp, n, sc.secrets(cp, 43))
    srs = _CASES[("srs", cp.name, n)]
    if ("lag", cp.name, n, qap) not in _CASES:   # one preparation serves every crafted circuit of the domain
        _CASES[("lag", cp.name, n, qap)] = g.prepare_srs_host(cp.name, srs, log_n=n.bit_length() - 1, qap=_red(g, qap))
    got = g.generate_parameters_from_lagrange_host(cp.name, mats, _CASES[("lag", cp.name, n, qap)], qap=_red(g, qap))
    sc.assert_keys_equal(got, g.generate_parameters_from_srs_host(cp.name, mats, srs, _red(g, qap)), which)


@CURVES
def test_save_and_load(g, cp, tmp_path):
    srs, mats, n = _case(g, cp, "syn2")
    lag = g.prepare_srs_host(cp.name, srs, matrices=mats, qap=g.CircomReduction)
    path = os.path.join(str(tmp_path), "lagrange.npz")
    lag.save(path)
    back = g.LagrangeSRS.load(path)
    assert (back.curve, back.log_n, back.qap) == (cp.name, lag.log_n, sc.CIRCOM)
    for name in ("u_g1", "alpha_u_g1", "beta_u_g1", "u_g2", "h_g1", "tau_g1_0", "alpha_g1_0", "beta_g1_0", "tau_g2_0", "beta_g2"):
        a, b = getattr(lag, name), getattr(back, name)
        assert a.shape == b.shape and b.dtype == np.uint64 and (a == b).all(), name
    sc.assert_keys_equal(g.generate_parameters_from_lagrange_host(cp.name, mats, back, qap=g.CircomReduction),
                         _srs_key(g, cp, sc.CIRCOM, "syn2", mats, srs), "loaded")


def test_refusals(g):
    cp = pm.BN254
    srs, mats, n = _case(g, cp, "syn4")       # a domain of 16
    small_srs, small_mats, _ = _case(g, cp, "syn2")
    lag = g.prepare_srs_host(cp.name, srs, matrices=mats)
    with pytest.raises(g.G16Error) as e:      # another reduction than the one asked for
        g.generate_parameters_from_lagrange_host(cp.name, mats, lag, qap=g.CircomReduction)
    assert e.value.status == 3 and "qap" in str(e.value)
    with pytest.raises(g.G16Error) as e:      # another domain than the circuit's
        g.generate_parameters_from_lagrange_host(cp.name, small_mats, lag)
    assert e.value.status == 2 and "2^4" in str(e.value) and "2^2" in str(e.value), str(e.value)
    bad = g.LagrangeSRS(**{**lag.__dict__, "qap": 2})
    with pytest.raises((g.G16Error, ValueError)):
        g.generate_parameters_from_lagrange_host(cp.name, mats, bad)
    fields = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
    for field, keep in (("tau_g1", 2 * n - 2), ("tau_g2", n - 1), ("alpha_tau_g1", n - 1), ("beta_tau_g1", n - 1)):
        short = g.SRS(cp.name, **{f: (getattr(srs, f)[:keep] if f == field else getattr(srs, f)) for f in fields})
        with pytest.raises(g.G16Error) as e:
            g.prepare_srs_host(cp.name, short, log_n=4)
        assert e.value.status == 2 and field in str(e.value), (field, str(e.value))
    with pytest.raises(ValueError):
        g.prepare_srs_host(cp.name, srs)                                  # neither a size nor a circuit
    with pytest.raises(ValueError):
        g.prepare_srs_host(cp.name, srs, log_n=4, matrices=mats)        # both
    with pytest.raises(ValueError):
        g.prepare_srs_host("bls12_381", srs, log_n=4)                    # another curve
