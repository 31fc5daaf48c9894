"""GPU tier: setup from an SRS on the MI355X.  The group transform against its host twin and on inputs with closed-form answers; the key
from an SRS plus one delta contribution against the toxic-waste path (generate_parameters_with_qap with gamma = 1, t = tau), field by
field and byte for byte, on circuits and on crafted matrices; the key in use (prove, verify); contribute_delta; refusals.  No
tolerance anywhere: affine Montgomery coordinates are canonical."""
import numpy as np
import pytest

import pymodel as pm
import srs_cases as sc
from helpers import arr_to_g1, arr_to_g2, circuit_from_pymodel, g1_to_arr, g2_to_arr, ints_to_mont

pytestmark = pytest.mark.gpu
QAPS = [sc.LIBSNARK, sc.CIRCOM]
QAP_IDS = ["libsnark", "circom"]


@pytest.fixture(scope="module")
def g():
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module")
def provers(g):
    """one Groth16 object per (curve, reduction), made on first use and closed with the module"""
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


def _secrets(orc, cp, seed=91):
    tau, alpha, beta, delta, delta2 = orc.rand_fr(cp.name, seed, 5)
    return tau, alpha, beta, delta, delta2


def _neg_points(cp, arr, g2):
    pts = (arr_to_g2 if g2 else arr_to_g1)(arr, cp)
    G = pm.groups(cp)[1 if g2 else 0]
    return (g2_to_arr if g2 else g1_to_arr)([G.neg(P) for P in pts], cp)


# ---- the transform -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 10])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_group_ntt_equals_host_twin(g, orc, provers, cp, g2, log_n):
    """both directions; from 8 points on the input carries identities and a point next to its negative"""
    n = 1 << log_n
    pts = orc.synth_bases(cp.name, g2, 100 + log_n, n)
    if n >= 8:
        pts[1::4] = 0
        pts[3] = _neg_points(cp, pts[2:3], g2)[0]
        pts[n - 1] = pts[n - 2]
    for inverse in (False, True):
        got = provers(cp).group_ntt(pts, inverse=inverse)
        assert (got == g.group_ntt_host(cp.name, pts, inverse=inverse)).all(), inverse


@pytest.mark.parametrize("log_n", [1, 3, 10])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_group_ntt_of_equal_points(orc, provers, cp, g2, log_n):
    """tau = 1: the first butterflies add P + P and subtract P - P; the inverse transform is [P, O, ..., O], the forward one [n P, O, ...]"""
    n = 1 << log_n
    P = orc.synth_bases(cp.name, g2, 5, 1)
    pts = np.repeat(P, n, axis=0)
    want = np.zeros_like(pts)
    want[0] = P[0]
    assert (provers(cp).group_ntt(pts, inverse=True) == want).all()
    fwd = provers(cp).group_ntt(pts, inverse=False)
    assert not fwd[1:].any() and fwd[0].any()
    assert (provers(cp).group_ntt(fwd, inverse=True) == pts).all()


@pytest.mark.parametrize("log_n", [3, 10])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_group_ntt_of_root_powers(provers, gens, cp, log_n):
    """the SRS of tau = w^m: L_i(w^m) is 1 at i = m and 0 elsewhere, so the inverse transform is the generator at index m alone"""
    n = 1 << log_n
    w = pm.Domain(cp, n).omega
    one = sc.fr(cp, 1)
    for m in (0, 1, n // 2, n - 1):
        srs = provers(cp).srs_from_trapdoor(n, sc.fr(cp, pow(w, m, cp.r)), one, one, gens[cp.name]["g1gen"], gens[cp.name]["g2gen"])
        for pts, gen in ((srs.tau_g1[:n], gens[cp.name]["g1gen"]), (srs.tau_g2, gens[cp.name]["g2gen"])):
            want = np.zeros_like(pts)
            want[m] = gen
            assert (provers(cp).group_ntt(np.ascontiguousarray(pts), inverse=True) == want).all(), m


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_group_ntt_of_alternating_signs(orc, provers, cp, g2):
    """[P, -P, P, -P, ...]: every first-stage sum cancels; the forward transform is n P at index n / 2 and the identity elsewhere"""
    n = 16
    P = orc.synth_bases(cp.name, g2, 9, 1)
    pts = np.repeat(P, n, axis=0)
    pts[1::2] = _neg_points(cp, P, g2)[0]
    fwd = provers(cp).group_ntt(pts, inverse=False)
    assert fwd[n // 2].any() and not np.delete(fwd, n // 2, axis=0).any()
    want = np.zeros_like(pts)
    want[n // 2] = P[0]
    assert (provers(cp).group_ntt(pts, inverse=True) == want).all()


# ---- the key -------------------------------------------------------------------------------------------------------------------------
def _circuit(orc, cp, name):
    if name.startswith("syn"):
        return orc.syn_circuit(cp.name, int(name[3:]), 3)
    if name == "mimc5":
        return circuit_from_pymodel(cp, *pm.mimc_circuit(cp, 5, 2))      # 10 + 2 rows in a domain of 16
    return circuit_from_pymodel(cp, *pm.syn_circuit(cp, 3, 1, dense=True))


def _both_ways(g, orc, prover, gens, cp, mats, label):
    """contribute_delta(generate_parameters_from_srs(srs_from_trapdoor)) against generate_parameters_with_qap(gamma = 1, t = tau)"""
    tau, alpha, beta, delta, _ = _secrets(orc, cp)
    g1, g2 = gens[cp.name]["g1gen"], gens[cp.name]["g2gen"]
    n = 1
    while n < mats.num_constraints + mats.num_instance_variables:
        n <<= 1
    srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
    got = prover.contribute_delta(prover.generate_parameters_from_srs(mats, srs), delta)
    want = prover.generate_parameters_with_qap(mats, alpha, beta, sc.fr(cp, 1), delta, g1, g2, tau)
    sc.assert_keys_equal(got, want, label)
    return got, srs


@pytest.mark.parametrize("name", ["syn2", "syn4", "syn10", "mimc5", "dense3"])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_key_from_srs_equals_toxic_waste_key(g, orc, provers, gens, cp, qap, name):
    _both_ways(g, orc, provers(cp, qap), gens, cp, sc.mats_of(g, _circuit(orc, cp, name)), name)


def _rows_mats(g, cp, ni, nv, rows_a, rows_b, rows_c):
    conv = lambda rows: [[(sc.fr(cp, cf), idx) for cf, idx in row] for row in rows]  # noqa: E731
    return g.ConstraintMatrices.from_rows(cp.name, ni, nv - ni, conv(rows_a), conv(rows_b), conv(rows_c))


def _crafted(g, cp, which):
    r = cp.r
    rng = pm.SplitMix64(17)
    big = [rng.field(r) for _ in range(8)]
    seg = int(g.lib().c.g16_srs_segment_len())
    if which == "coefficients":
        # zero coefficients, a repeated (row, column), 1, r - 1, 2, full-size, column 7 nowhere, column 5's terms cancel on row 2
        a = [[(1, 0), (0, 3), (2, 4)], [(r - 1, 2), (big[0], 3), (big[0], 3)], [(big[1], 5), (r - big[1], 5), (1, 1)], [(0, 6)], [(2, 2), (r - 2, 6)]]
        b = [[(1, 1)], [(big[2], 0), (1, 4)], [(r - 1, 4)], [(1, 6), (1, 6)], [(0, 0)]]
        c = [[(big[3], 6)], [(1, 2)], [(3, 5), (r - 3, 5)], [(big[4], 3)], [(1, 0), (r - 1, 1)]]
        return _rows_mats(g, cp, 2, 8, a, b, c)
    if which == "one_input":
        return _rows_mats(g, cp, 1, 4, [[(1, 1)], [(big[0], 2)], [(1, 3)]], [[(1, 2)], [(1, 0)], [(r - 1, 1)]], [[(1, 3)], [(big[1], 1)], [(2, 0)]])
    if which == "no_witness":     # num_variables = num_inputs: l_query is empty
        return _rows_mats(g, cp, 3, 3, [[(1, 1)], [(big[0], 2)]], [[(1, 2)], [(1, 0)]], [[(big[1], 0)], [(2, 1)]])
    nc = 4 * seg + 3                  # the constant-one column holds 4 segments and 3 entries more
    if which == "long_ones":
        a = [[(1, 0), (1, 2 + i % 3)] for i in range(nc)]
        b = [[(1, 0)] for _ in range(nc)]
        c = [[(1, 0), (1, 1)] for _ in range(nc)]
    else:                             # long_mixed: the same lengths with 1, r - 1, 0, 2 and full-size coefficients in turn
        cf = lambda i: (1, r - 1, 0, 2, big[i % 8], r - big[(i + 3) % 8])[i % 6]  # noqa: E731
        a = [[(cf(i), 0), (1, 2 + i % 3)] for i in range(nc)]
        b = [[(cf(i + 1), 0)] for i in range(nc)]
        c = [[(cf(i + 2), 0), (cf(i), 1)] for i in range(nc)]
    return _rows_mats(g, cp, 2, 5, a, b, c)


@pytest.mark.parametrize("which", ["coefficients", "one_input", "no_witness", "long_ones", "long_mixed"])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_crafted_matrices_equal_toxic_waste_key(g, orc, provers, gens, cp, qap, which):
    mats = _crafted(g, cp, which)
    got, _ = _both_ways(g, orc, provers(cp, qap), gens, cp, mats, which)
    if which == "coefficients":       # the unused variable and the cancelled column are the identity in every query they could appear in
        assert not got.a_query[7].any() and not got.b_g1_query[7].any() and not got.b_g2_query[7].any() and not got.l_query[7 - 2].any()
        assert not got.a_query[5].any()
    if which == "no_witness":
        assert got.l_query.shape[0] == 0


@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_srs_key_proves_and_verifies(g, orc, provers, gens, cp, qap):
    ck = orc.syn_circuit(cp.name, 6, 4)
    mats = sc.mats_of(g, ck)
    prover = provers(cp, qap)
    pk, _ = _both_ways(g, orc, prover, gens, cp, mats, "syn6")
    proof = prover.create_random_proof_with_reduction(pk, mats, ck.num_inputs, ck.num_constraints, ck.z)
    vk = g.VerifyingKey.from_proving_key(pk)
    good, bad = ck.z[1: ck.num_inputs], ck.z[2: 1 + ck.num_inputs]
    assert (good != bad).any()
    assert g.verify_proof_host(cp.name, vk, proof, good) and not g.verify_proof_host(cp.name, vk, proof, bad)
    pvk = prover.prepare_verifying_key(pk)
    assert prover.verify_proof(pvk, proof, good) and not prover.verify_proof(pvk, proof, bad)


# ---- contribute_delta ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_contribute_delta(g, orc, provers, gens, cp):
    prover = provers(cp)
    mats = _crafted(g, cp, "coefficients")       # l_query[5] is the identity (column 7 occurs nowhere)
    tau, alpha, beta, d1, d2 = _secrets(orc, cp, 33)
    srs = prover.srs_from_trapdoor(8, tau, alpha, beta, gens[cp.name]["g1gen"], gens[cp.name]["g2gen"])
    base = prover.generate_parameters_from_srs(mats, srs)
    base.h_query[2] = 0                              # and an identity among the h points
    before = {f: getattr(base, f).copy() for f in sc.KEY_FIELDS}
    two = prover.contribute_delta(prover.contribute_delta(base, d1), d2)
    d12 = ints_to_mont([pm.from_mont_limbs([int(x) for x in d1], cp.r) * pm.from_mont_limbs([int(x) for x in d2], cp.r) % cp.r], cp.r, 4)[0]
    once = prover.contribute_delta(base, d12.copy())
    sc.assert_keys_equal(two, once, "d1 then d2")
    assert not two.l_query[5].any() and not two.h_query[2].any()
    assert (two.delta_g1 != base.delta_g1).any() and (two.l_query[0] != base.l_query[0]).any()
    for f in sc.KEY_FIELDS:                          # the input key is untouched
        assert (getattr(base, f) == before[f]).all(), f
    for f in ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query"):
        assert (getattr(two, f) == before[f]).all(), f
    with pytest.raises(g.UnexpectedIdentity):
        prover.contribute_delta(base, np.zeros(4, dtype=np.uint64))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(g, orc, provers, gens):
    import ctypes as C

    cp = pm.BN254
    prover = provers(cp)
    mats = sc.mats_of(g, orc.syn_circuit(cp.name, 3, 2))   # a domain of 8
    n = 8
    tau, alpha, beta, _, _ = _secrets(orc, cp, 5)
    srs = prover.srs_from_trapdoor(n + 2, tau, alpha, beta, gens[cp.name]["g1gen"], gens[cp.name]["g2gen"])   # longer than needed
    fields = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
    cut = lambda **keep: g.SRS(cp.name, **{f: np.ascontiguousarray(getattr(srs, f)[:keep.get(f)]) for f in fields})  # noqa: E731
    exact = cut(tau_g1=2 * n - 1, tau_g2=n, alpha_tau_g1=n, beta_tau_g1=n)
    sc.assert_keys_equal(prover.generate_parameters_from_srs(mats, srs), prover.generate_parameters_from_srs(mats, exact), "longer SRS")
    for field, keep in (("tau_g1", 2 * n - 2), ("tau_g2", n - 1), ("alpha_tau_g1", n - 1), ("beta_tau_g1", n - 1)):
        with pytest.raises(g.G16Error) as e:
            prover.generate_parameters_from_srs(mats, cut(**{field: keep}))
        assert e.value.status == 2 and field in str(e.value), (field, str(e.value))
    lb, ctx = prover._ctx.lib, prover._ctx.handle
    from groth16_amd.groth16 import _blank_key, _csr_views, _params_view

    views, keep_alive = _csr_views(mats)
    blank = _blank_key(cp.name, g.LibsnarkReduction, mats)   # held to the end: the view keeps raw addresses only
    out = _params_view(blank)
    sv, keep_srs = exact.view()
    ni, nv = mats.num_instance_variables, mats.num_instance_variables + mats.num_witness_variables
    call = lambda qap, s, o: lb.c.g16_generate_parameters_srs(ctx, views, ni, mats.num_constraints, nv, qap, s, o)  # noqa: E731
    assert call(0, C.byref(sv), C.byref(out)) == 0 and blank.a_query.any() and blank.h_query.any()
    assert call(0, None, C.byref(out)) == 3 and call(0, C.byref(sv), None) == 3      # a null view: G16_ERR_BAD_ARG
    assert call(2, C.byref(sv), C.byref(out)) == 3                                   # qap = 2
    out.flags = 1                                                                    # G16_PARAMS_DEVICE_PTRS is refused
    assert call(0, C.byref(sv), C.byref(out)) == 3
    with pytest.raises(TypeError):
        prover.contribute_delta(g.DeviceProvingKey.__new__(g.DeviceProvingKey), sc.fr(cp, 2))
