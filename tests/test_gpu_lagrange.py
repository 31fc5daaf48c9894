"""GPU tier: the Lagrange form of an SRS on the MI355X (libg16_lagrange.so).  The transform on the windowed scalar multiplication
against the existing transform's host twin -- at the sizes where a stage changes shape, with a chunk boundary inside a wave and one
task per launch, on the edge inputs of lagrange_cases.py and on inputs with closed-form answers; the prepared arrays and the h
basis against the existing path; the key from the Lagrange form against the key from the SRS, field by field and byte for byte; the
key in use; a tampered Lagrange point caught by the key check; refusals.  No tolerance anywhere."""
import numpy as np
import pytest

import lagrange_cases as lc
import pymodel as pm
import srs_cases as sc

pytestmark = pytest.mark.gpu
QAPS = [sc.LIBSNARK, sc.CIRCOM]
QAP_IDS = ["libsnark", "circom"]
GROUPS = pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
CURVES = pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
LAGRANGE_FIELDS = ("u_g1", "alpha_u_g1", "beta_u_g1", "u_g2", "h_g1", "tau_g1_0", "alpha_g1_0", "beta_g1_0", "tau_g2_0", "beta_g2")


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


@pytest.fixture(scope="module")
def shared(g, orc, provers, gens):
    """what several tests need of the existing path, made once and left unchanged: the SRS of a domain (two points longer than it
    needs) and the key of generate_parameters_from_srs per (curve, reduction, circuit)"""
    srs, keys = {}, {}

    def get_srs(cp, n):
        if (cp.name, n) not in srs:
            tau, alpha, beta = orc.rand_fr(cp.name, 91, 3)
            srs[(cp.name, n)] = provers(cp).srs_from_trapdoor(n + 1, tau, alpha, beta, gens[cp.name]["g1gen"], gens[cp.name]["g2gen"])
        return srs[(cp.name, n)]

    def get_key(cp, qap, name, mats, n):
        if (cp.name, qap, name) not in keys:
            keys[(cp.name, qap, name)] = provers(cp, qap).generate_parameters_from_srs(mats, get_srs(cp, n))
        return keys[(cp.name, qap, name)]

    return get_srs, get_key


def _domain(mats):
    n = 1
    while n < mats.num_constraints + mats.num_instance_variables:
        n <<= 1
    return n


def _points(orc, cp, g2, n, seed):
    pts = orc.synth_bases(cp.name, g2, seed, n)
    if n >= 8:
        pts[1::4] = 0
        pts[n - 1] = pts[n - 2]
    return pts


# ---- the transform -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 8])
@GROUPS
@CURVES
def test_windowed_transform_equals_host_twin_of_the_existing_one(g, orc, provers, cp, g2, log_n):
    """1: the last stage is stage 0 (all twiddle 1, the scale alone); 2 and 3: stage 0 with the scale, a stage with a single multiplying
    butterfly per block; 8: 128 butterflies, one 128-lane workgroup of G1 tasks and two of G2 lane pairs"""
    pts = _points(orc, cp, g2, 1 << log_n, 400 + log_n)
    for inverse in (False, True):
        got = provers(cp).group_ntt_windowed(pts, inverse=inverse)
        assert (got == g.group_ntt_host(cp.name, pts, inverse=inverse)).all(), inverse


@pytest.mark.parametrize("chunk", [48, 1])
@GROUPS
@CURVES
def test_chunk_boundaries(g, orc, provers, monkeypatch, cp, g2, chunk):
    """64 points, 32 butterflies a stage (64 lanes of G2 pairs): a chunk of 48 holds a whole stage, a chunk of 20 -- run beside it -- cuts
    every stage inside a wave (launches of 20 and 12 tasks, the multiplications of a chunk counted from the butterflies before
    it), a chunk of 1 gives one task per launch"""
    pts = _points(orc, cp, g2, 64, 77)
    want = {inv: g.group_ntt_host(cp.name, pts, inverse=inv) for inv in (False, True)}
    for c in (chunk, 20) if chunk == 48 else (chunk,):
        monkeypatch.setenv("G16_LAGRANGE_CHUNK", str(c))
        for inverse in (False, True):
            assert (provers(cp).group_ntt_windowed(pts, inverse=inverse) == want[inverse]).all(), (c, inverse)


@pytest.mark.parametrize("log_n", lc.LOG_NS)
@GROUPS
@CURVES
def test_edge_inputs(g, provers, cp, g2, log_n):
    for label, pts in lc.edge_inputs(cp.name, g2, log_n):
        arr = lc.to_array(cp.name, g2, pts)
        for inverse in (False, True):
            got = provers(cp).group_ntt_windowed(arr, inverse=inverse)
            assert (got == g.group_ntt_host(cp.name, arr, inverse=inverse)).all(), (label, inverse)


@pytest.mark.parametrize("log_n", [3, 6])
@CURVES
def test_transform_of_root_powers(provers, gens, cp, log_n):
    """the SRS of tau = w^m: L_i(w^m) is 1 at i = m and 0 elsewhere, so the inverse transform is the generator at index m alone"""
    n = 1 << log_n
    w = pm.Domain(cp, n).omega
    one = sc.fr(cp, 1)
    for m in (0, 1, n // 2, n - 1):
        srs = provers(cp).srs_from_trapdoor(n, sc.fr(cp, pow(w, m, cp.r)), one, one, gens[cp.name]["g1gen"], gens[cp.name]["g2gen"])
        for pts, gen in ((srs.tau_g1[:n], gens[cp.name]["g1gen"]), (srs.tau_g2, gens[cp.name]["g2gen"])):
            want = np.zeros_like(pts)
            want[m] = gen
            assert (provers(cp).group_ntt_windowed(np.ascontiguousarray(pts), inverse=True) == want).all(), m


# ---- the Lagrange form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [2, 6])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@CURVES
def test_prepared_arrays_and_h_basis(g, orc, provers, shared, cp, qap, log_n):
    get_srs, get_key = shared
    n = 1 << log_n
    ck = orc.syn_circuit(cp.name, log_n, 3)
    mats = sc.mats_of(g, ck)
    assert _domain(mats) == n
    srs = get_srs(cp, n)
    prover = provers(cp, qap)
    lag = prover.prepare_srs(srs, matrices=mats)
    assert (lag.curve, lag.log_n, lag.qap) == (cp.name, log_n, qap)
    for name, src in (("u_g1", srs.tau_g1), ("alpha_u_g1", srs.alpha_tau_g1), ("beta_u_g1", srs.beta_tau_g1), ("u_g2", srs.tau_g2)):
        assert (getattr(lag, name) == prover.group_ntt(np.ascontiguousarray(src[:n]), inverse=True)).all(), name
    key = get_key(cp, qap, "syn%d" % log_n, mats, n)
    assert lag.h_g1.shape == key.h_query.shape and (lag.h_g1 == key.h_query).all()
    tm = prover.lagrange_timings()
    assert all(tm[k] > 0 for k in ("u_g1_ms", "alpha_u_g1_ms", "beta_u_g1_ms", "u_g2_ms")), tm
    if log_n == 2:   # the host twin makes the same object
        host = g.prepare_srs_host(cp.name, srs, log_n=log_n, qap=prover.qap)
        for name in LAGRANGE_FIELDS:
            assert (getattr(host, name) == getattr(lag, name)).all(), name


# ---- the key from it -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [6, 8])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@CURVES
def test_key_from_lagrange_equals_key_from_srs(g, orc, provers, shared, cp, qap, k):
    get_srs, get_key = shared
    ck = orc.syn_circuit(cp.name, k, 3)
    mats = sc.mats_of(g, ck)
    n = _domain(mats)
    prover = provers(cp, qap)
    lag = prover.prepare_srs(get_srs(cp, n), log_n=k)
    got = prover.generate_parameters_from_lagrange(mats, lag)
    sc.assert_keys_equal(got, get_key(cp, qap, "syn%d" % k, mats, n), "syn%d" % k)
    assert prover.lagrange_timings()["products_ms"] > 0
    if k == 6:   # after one delta contribution the key proves and verifies
        pk = prover.contribute_delta(got, orc.rand_fr(cp.name, 5, 1)[0])
        proof = prover.create_random_proof_with_reduction(pk, mats, ck.num_inputs, ck.num_constraints, ck.z)
        good, bad = ck.z[1: ck.num_inputs], ck.z[2: 1 + ck.num_inputs]
        assert (good != bad).any()
        pvk = prover.prepare_verifying_key(pk)
        assert prover.verify_proof(pvk, proof, good) and not prover.verify_proof(pvk, proof, bad)


@pytest.mark.parametrize("group", [("coefficients", "no_witness"), ("long_ones",)], ids=["two circuits", "long_ones"])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@CURVES
def test_crafted_matrices_and_one_form_for_two_circuits(g, provers, shared, cp, qap, group):
    """the crafted matrices of the existing path's tests: an empty column and coefficients 0, 1 and r - 1 in two different circuits of
    a domain of 8, both keys from ONE Lagrange form; a constant-one column above four segments of the sparse product (domain 256; its
    mixed-coefficient sibling runs on the CPU tier, where the existing path's key costs less)"""
    import test_gpu_srs as tgs

    get_srs, get_key = shared
    prover = provers(cp, qap)
    mats = [tgs._crafted(g, cp, which) for which in group]
    n = _domain(mats[0])
    assert all(_domain(m) == n for m in mats)
    lag = prover.prepare_srs(get_srs(cp, n), log_n=n.bit_length() - 1)
    before = {f: getattr(lag, f).copy() for f in LAGRANGE_FIELDS}
    for which, m in zip(group, mats):
        sc.assert_keys_equal(prover.generate_parameters_from_lagrange(m, lag), get_key(cp, qap, which, m, n), which)
    for f in LAGRANGE_FIELDS:   # the form is read, never written
        assert (getattr(lag, f) == before[f]).all(), f


@CURVES
def test_a_replaced_lagrange_point_fails_the_key_check(g, orc, provers, shared, cp):
    get_srs, get_key = shared
    ck = orc.syn_circuit(cp.name, 4, 3)
    mats = sc.mats_of(g, ck)
    n = _domain(mats)
    prover = provers(cp)
    srs = get_srs(cp, n)
    lag = prover.prepare_srs(srs, matrices=mats)
    honest = prover.generate_parameters_from_lagrange(mats, lag)
    assert prover.check_key_derivation(mats, srs, honest)
    a = ck.abc[0]
    row = next(i for i in range(ck.num_constraints) if a.row_ptr[i + 1] > a.row_ptr[i] and a.val[a.row_ptr[i]].any())
    lag.u_g1[row] = lag.u_g1[(row + 1) % n]
    forged = prover.generate_parameters_from_lagrange(mats, lag)
    assert (forged.a_query != honest.a_query).any()
    res = prover.check_key_derivation(mats, srs, forged)
    assert not res and "A" in res.failed, res


def test_refusals(g, orc, provers, shared):
    get_srs, _ = shared
    cp = pm.BN254
    prover = provers(cp)
    mats = sc.mats_of(g, orc.syn_circuit(cp.name, 3, 2))      # a domain of 8
    small = sc.mats_of(g, orc.syn_circuit(cp.name, 2, 2))
    n = 8
    srs = get_srs(cp, n)
    lag = prover.prepare_srs(srs, matrices=mats)
    with pytest.raises(g.G16Error) as e:                        # prepared for Libsnark, asked of a Circom object
        provers(cp, sc.CIRCOM).generate_parameters_from_lagrange(mats, lag)
    assert e.value.status == 3 and "qap" in str(e.value)
    with pytest.raises(g.G16Error) as e:                        # another domain than the circuit's
        prover.generate_parameters_from_lagrange(small, lag)
    assert e.value.status == 2 and "2^3" in str(e.value) and "2^2" in str(e.value), str(e.value)
    fields = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
    for field, keep in (("tau_g1", 2 * n - 2), ("tau_g2", n - 1), ("alpha_tau_g1", n - 1), ("beta_tau_g1", n - 1)):
        short = g.SRS(cp.name, **{f: np.ascontiguousarray(getattr(srs, f)[:keep] if f == field else getattr(srs, f)) for f in fields})
        with pytest.raises(g.G16Error) as e:
            prover.prepare_srs(short, log_n=3)
        assert e.value.status == 2 and field in str(e.value), (field, str(e.value))
    with pytest.raises(ValueError):
        prover.prepare_srs(srs)
    with pytest.raises(ValueError):
        prover.group_ntt_windowed(np.zeros((3, 8), dtype=np.uint64))
