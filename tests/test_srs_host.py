"""CPU tier: setup from an SRS through the host twins (g16_host_group_ntt, g16_host_generate_parameters_srs) -- the same butterflies
and the same sums the kernels run, compiled for the host -- against the literal big-int model of srs_cases.py and against the key
made in the exponent from the toxic waste with gamma = delta = 1.  Every comparison is bit for bit."""
import numpy as np
import pytest

import pymodel as pm
import srs_cases as sc
from helpers import g1_to_arr, g2_to_arr


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


def _points(cp, g2, n, seed):
    """n points with their discrete logs; a few identities and a P, -P pair among them when there is room"""
    G = pm.groups(cp)[1 if g2 else 0]
    gen = cp.g2 if g2 else cp.g1
    rng = pm.SplitMix64(seed)
    ks = [rng.field(cp.r) for _ in range(n)]
    if n >= 4:
        ks[1], ks[3] = 0, (-ks[2]) % cp.r
    return ks, [G.mul(gen, k) if k else None for k in ks]


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_host_group_ntt_matches_dft_sum(g, cp, g2, log_n):
    n = 1 << log_n
    G = pm.groups(cp)[1 if g2 else 0]
    conv = g2_to_arr if g2 else g1_to_arr
    _, pts = _points(cp, g2, n, 7 + log_n)
    arr = conv(pts, cp)
    dom = pm.Domain(cp, n)
    fwd = g.group_ntt_host(cp.name, arr, inverse=False)
    assert (fwd == conv(sc.model_group_dft(G, pts, dom.omega, cp.r), cp)).all()
    inv = g.group_ntt_host(cp.name, arr, inverse=True)
    assert (inv == conv(sc.model_group_dft(G, pts, dom.omega_inv, cp.r, dom.n_inv), cp)).all()
    assert (g.group_ntt_host(cp.name, fwd, inverse=True) == arr).all()
    assert (g.group_ntt_host(cp.name, inv, inverse=False) == arr).all()


_MODEL = {}


def _case(g, cp, name, cs, z):
    """the SRS and the flat circuit of a case, built once per curve and circuit"""
    key = (cp.name, name)
    if key not in _MODEL:
        sec = sc.secrets(cp)
        srs = sc.model_srs(cp, sc.domain_size(cs), sec)
        _MODEL[key] = (sec, srs, sc.srs_to_arrays(g, cp, srs), sc.mats_of(g, sc.flat(cp, cs, z)))
    return _MODEL[key]


@pytest.mark.parametrize("qap", [sc.LIBSNARK, sc.CIRCOM], ids=["libsnark", "circom"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_host_key_from_srs_matches_model_and_trapdoor(g, cp, qap):
    red = g.LibsnarkReduction if qap == sc.LIBSNARK else g.CircomReduction
    for name, cs, z in sc.host_circuits(cp):
        sec, srs, srs_arr, mats = _case(g, cp, name, cs, z)
        got = g.generate_parameters_from_srs_host(cp.name, mats, srs_arr, red)
        sc.assert_keys_equal(got, sc.key_to_arrays(cp, sc.trapdoor_key(cp, cs, sec, qap)), (name, "trapdoor"))
        sc.assert_keys_equal(got, sc.key_to_arrays(cp, sc.model_key_from_srs(cp, cs, srs, qap)), (name, "model"))


def test_host_refusals(g):
    cp = pm.BN254
    name, cs, z = next(sc.host_circuits(cp))
    sec, srs, srs_arr, mats = _case(g, cp, name, cs, z)
    n = sc.domain_size(cs)
    for field, keep in (("tau_g1", 2 * n - 2), ("tau_g2", n - 1), ("alpha_tau_g1", n - 1), ("beta_tau_g1", n - 1)):
        short = g.SRS(cp.name, **{f: (getattr(srs_arr, f)[:keep] if f == field else getattr(srs_arr, f))
                                  for f in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")})
        with pytest.raises(g.G16Error) as e:
            g.generate_parameters_from_srs_host(cp.name, mats, short)
        assert e.value.status == 2 and field in str(e.value), (field, str(e.value))

    class Qap2:
        QAP_ID = 2
        h_query_len = staticmethod(lambda n: n)

    with pytest.raises(g.G16Error) as e:
        g.generate_parameters_from_srs_host(cp.name, mats, srs_arr, Qap2)
    assert e.value.status == 3
    assert int(g.lib().c.g16_srs_segment_len()) >= 8
