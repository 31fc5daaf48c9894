"""GPU tier: the fixed-base kernels in place (fixed_base_table_kernel, fixed_base_mul_kernel of csrc/setup.hip), through the public
entry points alone.  srs_from_trapdoor is the source of every SRS of the SRS, ceremony, phase-1, key-check and Lagrange suites and
generate_parameters_with_qap the expected value of every key derived from one; their own tests feed them random scalars.  Here the
scalars are chosen (tests/fixed_base_cases.py): the identity, 1, r - 1, every byte 255, one non-zero byte at every position; single
table entries d * 2^(8 w) * G read on their own; array lengths 1, 63, 64, 65 and 127 with zero scalars and alternating signs; a
crafted matrix whose queries are chosen multiples.  Expected values are pymodel's k G, k reduced mod r by the model; no tolerance:
affine Montgomery coordinates are canonical."""
import numpy as np
import pytest

import fixed_base_cases as fb
import pymodel as pm
import srs_cases as sc
from helpers import g1_to_arr, g2_to_arr

pytestmark = pytest.mark.gpu
CURVES = ("bls12_381", "bn254")


@pytest.fixture(scope="module")
def provers():
    import groth16_amd

    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = groth16_amd.Groth16(curve, 0)
        return made[curve]

    yield get
    for p in made.values():
        p.close()


def gen_arrays(curve):
    cp = pm.CURVES[curve]
    g1, g2 = fb.gens(curve)
    return g1_to_arr([g1], cp)[0], g2_to_arr([g2], cp)[0]


def make_srs(provers, curve, n, tau, alpha, beta):
    cp = pm.CURVES[curve]
    g1, g2 = gen_arrays(curve)
    return provers(curve).srs_from_trapdoor(n, sc.fr(cp, tau), sc.fr(cp, alpha), sc.fr(cp, beta), g1, g2)


def assert_srs(curve, srs, want, label):
    cp = pm.CURVES[curve]
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"):
        w = (g2_to_arr if name.endswith("g2") else g1_to_arr)(want[name], cp)
        got = np.asarray(getattr(srs, name)).reshape(w.shape)
        bad = np.flatnonzero((got != w).any(axis=1))
        assert not len(bad), "%s: %s[%d] is not the model's multiple" % (label, name, int(bad[0]))


@pytest.mark.parametrize("curve", CURVES)
def test_single_scalars(provers, curve):
    """n = 1, tau = 1: alpha through the G1 kernel, beta through the G1 and the G2 kernel, one lane each"""
    ks = fb.single_scalars(curve)
    for i, (name, k) in enumerate(ks):
        alpha = ks[(i + 7) % len(ks)][1]
        srs = make_srs(provers, curve, 1, 1, alpha, k)
        assert_srs(curve, srs, fb.expected_srs(curve, 1, 1, alpha, k), "beta = %s, alpha = %s" % (name, ks[(i + 7) % len(ks)][0]))
        if k == 0:
            assert not srs.beta_g2.any() and not srs.beta_tau_g1.any()     # the identity: all-zero words


@pytest.mark.parametrize("curve", CURVES)
def test_single_table_entries(provers, curve):
    """n = 32, tau = 256: alpha_tau_g1[w] = d 256^w G and beta_tau_g1[w] = d' 256^w G are single table entries for w < 31, tau_g2[w]
    is entry w * 255 of the G2 table; window 31 and tau_g1's powers past it wrap mod r"""
    for d, d2 in fb.window_cases(curve):
        srs = make_srs(provers, curve, 32, 256, d, d2)
        assert_srs(curve, srs, fb.expected_srs(curve, 32, 256, d, d2), "d = %d, d' = %d" % (d, d2))


@pytest.mark.parametrize("curve", CURVES)
def test_array_lengths(provers, curve):
    for n, tau, alpha, beta, what in fb.size_cases(curve):
        srs = make_srs(provers, curve, n, tau, alpha, beta)
        assert_srs(curve, srs, fb.expected_srs(curve, n, tau, alpha, beta), "n = %d, %s" % (n, what))
        if tau == 0:
            assert not srs.tau_g1[1:].any() and not srs.tau_g2[1:].any() and srs.tau_g1[0].any()


@pytest.mark.parametrize("num_witness", [None, 0, 1], ids=["targets", "no-witness", "one-witness"])
@pytest.mark.parametrize("curve", CURVES)
def test_crafted_queries(provers, curve, num_witness):
    """generate_parameters_with_qap on single-entry columns with the coefficient target * u_i(t)^-1: a_query, b_g1_query and b_g2_query
    are target * G for the targets 0, 1, r - 1 and every byte 255; an unused variable; an empty l_query and one with a single entry.
    The whole key is compared with the key in the exponent (srs_cases.trapdoor_key, gamma = 1)."""
    import groth16_amd

    cp = pm.CURVES[curve]
    sec = dict(sc.secrets(cp, 77))
    sec["g1"], sec["g2"] = fb.gens(curve)
    cs, want = fb.qap_circuit(curve, sec["tau"], num_witness)
    ck = sc.flat(cp, cs, [1] + [0] * cs.num_witness)
    g1, g2 = gen_arrays(curve)
    key = provers(curve).generate_parameters_with_qap(sc.mats_of(groth16_amd, ck), sc.fr(cp, sec["alpha"]), sc.fr(cp, sec["beta"]), sc.fr(cp, 1),
                                                      sc.fr(cp, sec["delta"]), g1, g2, sc.fr(cp, sec["tau"]))
    for col, target in want.items():
        w1 = g1_to_arr([fb.multiple(curve, 0, target)], cp)[0]
        w2 = g2_to_arr([fb.multiple(curve, 1, target)], cp)[0]
        assert (key.a_query[col] == w1).all() and (key.b_g1_query[col] == w1).all() and (key.b_g2_query[col] == w2).all(), (col, hex(target))
    nv = cs.num_inputs + cs.num_witness
    assert key.a_query.shape[0] == nv and key.l_query.shape[0] == cs.num_witness
    if num_witness is None:
        assert not key.a_query[nv - 1].any() and not key.b_g2_query[nv - 1].any() and not key.l_query[-1].any()   # the unused variable
    sc.assert_keys_equal(key, sc.key_to_arrays(cp, sc.trapdoor_key(cp, cs, sec, sc.LIBSNARK, sec["delta"])), curve)
