"""GPU tier: the ceremony checks on the MI355X.  rlc_sums against its host twin (byte for byte, through the digit kernel's block
border and every coefficient edge case) and against the existing MSM with the coefficients widened to Fr; check_srs against the flag
sets ceremony_cases.py derives in the exponent and against the host twin; check_delta_contribution / check_parameters on keys made
by generate_parameters_from_srs + contribute_delta; length handling, check=True, determinism.  No tolerance anywhere."""
import numpy as np
import pytest

import ceremony_cases as cc
import pymodel as pm
import srs_cases as sc
from helpers import arr_to_g1, circuit_from_pymodel, g1_to_arr, ints_to_mont

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


def _srs_copy(g, srs, **repl):
    return g.SRS(srs.curve, **{f: np.ascontiguousarray(repl.get(f, getattr(srs, f))).copy() for f in SRS_FIELDS})


def _double_row(cp, arr, idx):
    P = arr_to_g1(arr[idx:idx + 1], cp)[0]
    return g1_to_arr([pm.groups(cp)[0].add(P, P)], cp)[0]


# ---- the unit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_rlc_sums_equal_host_twin(g, orc, provers, cp, g2, n):
    """257 points are 256 coefficients: one full block of the digits kernel; 258 would start the next, 256 and 255 stop short of it"""
    prover = provers(cp)
    pts = orc.synth_bases(cp.name, g2, 200 + n, n + 1)[:n]
    if n >= 8:
        pts[5] = 0                      # an identity among the points
        pts[7] = pts[6]                 # a repeated point
    m = max(n - 1, 1)
    cases = cc.coeff_edge_cases(m)
    c = g.rlc_plan(m)["window_bits"]
    cases[f"windows_plan_c{c}"] = [cc.digit_coeff(c)] * m
    for label, co in cases.items():
        co = cc.coeff_array(co[:n - 1])
        lo, hi = prover.rlc_sums(pts, co)
        if n > 1:
            tm = prover.timings()
            assert tm["window_bits"] == c and tm["windows"] == g.rlc_plan(m)["windows"], label
        hlo, hhi = g.rlc_sums_host(cp.name, pts, co)
        assert (lo == hlo).all() and (hi == hhi).all(), (label, n)
    if n == 1:
        assert not lo.any() and not hi.any()
    if n >= 3:
        co = cc.random_coeffs(n - 1)
        co[n - 2] = 0
        with pytest.raises(g.G16Error) as e:
            prover.rlc_sums(pts, co)
        assert e.value.status == 3
        prover.rlc_sums(pts, None)


@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_rlc_sums_equal_existing_msm_past_one_chunk(g, orc, provers, cp):
    """more coefficients than one histogram / scatter workgroup takes (the plan's chunk, read from the plan), so two workgroups feed one
    bucket; against two calls of the existing MSM over the shifted slices, the coefficients widened to Fr"""
    prover = provers(cp)
    chunk = g.rlc_plan(2048)["chunk"]
    n = chunk + 300
    assert g.rlc_plan(n - 1)["chunk"] < n - 1, "the case no longer spans two workgroups"
    pts = orc.synth_bases(cp.name, False, 77, n)
    co = cc.random_coeffs(n - 1, 5)
    co[0], co[1], co[n - 2] = (1 << 128) - 1, 1, 1 << 127
    lo, hi = prover.rlc_sums(pts, co)
    fr = ints_to_mont(co, cp.r, 4)
    assert (lo == prover.msm(pts[:n - 1], fr)).all()
    assert (hi == prover.msm(np.ascontiguousarray(pts[1:]), fr)).all()


_FIRST_WORK_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import groth16_amd as g
pts, co = np.load(sys.argv[2]), np.load(sys.argv[3])
with g.Groth16("bls12_381", 0) as prover:
    lo, hi = prover.rlc_sums(pts, co)
    tm = prover.timings()
assert tm["window_bits"] == 16, tm
np.save(sys.argv[4], np.stack([lo, hi]))
"""


def test_rlc_sums_as_first_gpu_work_with_128_kib_histograms(g, orc, tmp_path):
    """G16_MSM_WINDOW=16 gives sort_digit_planes histograms of 2^15 counters, 128 KiB of dynamic LDS, which the count and scatter
    kernels may take only once their limit is raised.  In a fresh process whose first GPU work is rlc_sums no other sort has raised it
    before: 258 G1 points, 257 coefficients (one more than a block of the digits kernel), the sums against the host twin."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pts = orc.synth_bases("bls12_381", False, 1616, 258)
    co = cc.random_coeffs(257, 16)
    co[0], co[1], co[256] = (1 << 128) - 1, 1, 1 << 127
    co = cc.coeff_array(co)
    files = [str(tmp_path / name) for name in ("pts.npy", "co.npy", "sums.npy")]
    np.save(files[0], pts)
    np.save(files[1], co)
    run = subprocess.run([sys.executable, "-c", _FIRST_WORK_CHILD, root] + files, env=dict(os.environ, G16_MSM_WINDOW="16"),
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    lo, hi = np.load(files[2])
    hlo, hhi = g.rlc_sums_host("bls12_381", pts, co)
    assert (lo == hlo).all() and (hi == hhi).all()


# ---- the SRS -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_check_srs_flags(g, provers, cp, n):
    prover = provers(cp)
    coeffs = cc.random_coeffs(2 * n - 2)
    for label, srs, expect, where in cc.srs_cases(cp.name, n):
        arr = sc.srs_to_arrays(g, cp, srs)
        res = prover.check_srs(arr, coeffs)
        cc.assert_result(res, expect, where, label)
        host = g.check_srs_host(cp.name, arr, coeffs)
        assert (res.flags, res.array, res.index, res.reason) == (host.flags, host.array, host.index, host.reason), label


@pytest.fixture(scope="module")
def big_srs(g, orc, provers, gens):
    """the SRS of a domain of 2^10 points per curve, made on the GPU, and the tau_g2 of another tau"""
    made = {}

    def get(cp):
        if cp.name not in made:
            tau, alpha, beta, tau2 = orc.rand_fr(cp.name, 91, 4)
            g1, g2 = gens[cp.name]["g1gen"], gens[cp.name]["g2gen"]
            srs = provers(cp).srs_from_trapdoor(1 << 10, tau, alpha, beta, g1, g2)
            other = provers(cp).srs_from_trapdoor(1 << 10, tau2, alpha, beta, g1, g2)
            made[cp.name] = (srs, other.tau_g2)
        return made[cp.name]

    return get


@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_check_srs_at_2_10(g, provers, big_srs, cp):
    """tau_g1 (2047 points) is longer than tau_g2 (1024): the shared sort's entries beyond a shorter array are skipped"""
    prover = provers(cp)
    srs, tau_g2_other = big_srs(cp)
    N1 = len(srs.tau_g1)
    assert N1 == 2047 and len(srs.tau_g2) == 1024
    coeffs = cc.random_coeffs(N1 - 1, 3)
    cc.assert_result(prover.check_srs(srs, coeffs), set(), None, "honest")
    cc.assert_result(prover.check_srs(srs), set(), None, "honest, fresh coefficients")
    last = _srs_copy(g, srs)
    last.tau_g1[N1 - 1] = _double_row(cp, srs.tau_g1, N1 - 1)
    cc.assert_result(prover.check_srs(last, coeffs), {cc.TAU_G1}, None, "last index")
    swap = _srs_copy(g, srs)
    swap.tau_g1[[1500, 1501]] = srs.tau_g1[[1501, 1500]]
    cc.assert_result(prover.check_srs(swap, coeffs), {cc.TAU_G1}, None, "adjacent swap")
    wrong = _srs_copy(g, srs, tau_g2=tau_g2_other)
    assert (wrong.tau_g2[0] == srs.tau_g2[0]).all() and (wrong.tau_g2[1] != srs.tau_g2[1]).any()
    cc.assert_result(prover.check_srs(wrong, coeffs), {cc.TAU_G1, cc.TAU_G2, cc.ALPHA, cc.BETA}, None, "tau_g2 from tau'")


@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_check_srs_length_handling(g, orc, provers, cp):
    prover = provers(cp)
    n, extra = 4, 3
    sec = sc.secrets(cp)
    model = sc.model_srs(cp, n, sec, extra)
    assert len(model["tau_g1"]) == 2 * n - 1 + extra
    srs = sc.srs_to_arrays(g, cp, model)
    coeffs = cc.random_coeffs(len(model["tau_g1"]) - 1)
    cc.assert_result(prover.check_srs(srs, coeffs), set(), None, "longer than the domain needs")
    # an error beyond the prefix a domain of n points would use: the derivation never reads it, the check still fails
    bad = _srs_copy(g, srs)
    bad.tau_g1[2 * n] = _double_row(cp, srs.tau_g1, 2 * n)
    cc.assert_result(prover.check_srs(bad, coeffs), {cc.TAU_G1}, None, "beyond the prefix")
    name, cs, z = next(sc.host_circuits(cp))
    assert sc.domain_size(cs) == n
    mats = sc.mats_of(g, circuit_from_pymodel(cp, cs, z))
    sc.assert_keys_equal(prover.generate_parameters_from_srs(mats, bad), prover.generate_parameters_from_srs(mats, srs), "prefix")
    with pytest.raises(g.BadSRS) as e:
        prover.generate_parameters_from_srs(mats, bad, check=True)
    assert e.value.result.failed == ("TAU_G1",)
    sc.assert_keys_equal(prover.generate_parameters_from_srs(mats, srs, check=True), prover.generate_parameters_from_srs(mats, srs), "check=True")
    # refusals: an array too short for one equation, too few coefficients, a zero coefficient, the other curve's SRS
    with pytest.raises(g.G16Error) as e:
        prover.check_srs(_srs_copy(g, srs, tau_g2=srs.tau_g2[:1]))
    assert e.value.status == 2 and "tau_g2" in str(e.value)
    with pytest.raises(g.G16Error) as e:
        prover.check_srs(srs, coeffs[:-1])
    assert e.value.status == 2
    with pytest.raises(g.G16Error) as e:
        prover.check_srs(srs, coeffs[:-1] + [0])
    assert e.value.status == 3
    with pytest.raises(ValueError):
        prover.check_srs(g.SRS("bn254" if cp.name != "bn254" else "bls12_381", *[getattr(srs, f) for f in SRS_FIELDS]))


# ---- keys ----------------------------------------------------------------------------------------------------------------------
def _circuit(orc, cp, name):
    if name.startswith("syn"):
        return orc.syn_circuit(cp.name, int(name[3:]), 3)
    return circuit_from_pymodel(cp, *pm.mimc_circuit(cp, 5, 2))


@pytest.mark.parametrize("name", ["syn4", "mimc5", "syn10"])
@pytest.mark.parametrize("qap", QAPS, ids=QAP_IDS)
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_check_delta_contribution_and_parameters(g, orc, provers, gens, cp, qap, name):
    prover = provers(cp, qap)
    mats = sc.mats_of(g, _circuit(orc, cp, name))
    n = 1
    while n < mats.num_constraints + mats.num_instance_variables:
        n <<= 1
    tau, alpha, beta, d1, d2, tau2 = orc.rand_fr(cp.name, 57, 6)
    g1, g2 = gens[cp.name]["g1gen"], gens[cp.name]["g2gen"]
    srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
    k0 = prover.generate_parameters_from_srs(mats, srs)
    k1 = prover.contribute_delta(k0, d1)
    k2 = prover.contribute_delta(k1, d2)
    coeffs = cc.random_coeffs(max(len(k0.l_query), len(k0.h_query), 2 * n - 2), 13)   # enough for the key's sums and for the SRS
    for before, after in ((k0, k1), (k1, k2), (k0, k2)):     # one and two contributions, against the predecessor and the delta = 1 key
        cc.assert_result(prover.check_delta_contribution(before, after, coeffs), set(), None, (name, "honest"))
    cc.assert_result(prover.check_delta_contribution(k0, k2), set(), None, (name, "honest, fresh coefficients"))
    for i, (label, bad, expect, where) in enumerate(cc.key_tamper_cases(g, cp, k2)):
        cc.assert_result(prover.check_delta_contribution(k1, bad, coeffs), expect, where, (name, label))
        if name != "syn10" and i < 3:
            cc.assert_result(g.check_delta_contribution_host(cp.name, k1, bad, coeffs), expect, where, (name, label, "host"))
    cc.assert_result(prover.check_parameters(mats, srs, k2, coeffs), set(), None, (name, "check_parameters"))
    # the same key against another honest SRS (another tau, the same generators): alpha_g1 = alpha g1 still agrees, the first query
    # point that depends on tau does not, and l / h of the derived key belong to the other tau; the deltas chain from the same generators
    other = prover.srs_from_trapdoor(n, tau2, alpha, beta, g1, g2)
    res = prover.check_parameters(mats, other, k2, coeffs)
    assert set(res.failed) == {cc.FIXED_PART, cc.L, cc.H} and not res, (name, res.failed)
    assert res.array in cc.KEY_FIXED_NAMES and res.array not in ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2"), res.array
    # a tampered SRS stops check_parameters at the SRS
    bad_srs = _srs_copy(g, srs)
    bad_srs.tau_g1[len(srs.tau_g1) - 1] = _double_row(cp, srs.tau_g1, len(srs.tau_g1) - 1)
    res = prover.check_parameters(mats, bad_srs, k2)
    assert res.failed == ("TAU_G1",)
    with pytest.raises(ValueError):                  # keys of different shapes
        cut = cc.key_copy(g, k2)
        cut.h_query = cut.h_query[:-1]
        prover.check_delta_contribution(k1, cut)


# ---- determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cp", sc.CURVES, ids=lambda c: c.name)
def test_determinism(g, provers, cp):
    prover = provers(cp)
    cases = {label: (srs, expect, where) for label, srs, expect, where in cc.srs_cases(cp.name, 16)}
    coeffs = cc.random_coeffs(30, 21)
    for label in ("two bad points in one array", "tau_g2 from tau'", "tau_g1[last] doubled"):
        srs, expect, where = cases[label]
        arr = sc.srs_to_arrays(g, cp, srs)
        first = prover.check_srs(arr, coeffs)
        for _ in range(3):
            again = prover.check_srs(arr, coeffs)
            assert (again.flags, again.array, again.index, again.reason) == (first.flags, first.array, first.index, first.reason), label
        for _ in range(2):                           # fresh coefficients: a tampered SRS fails every time
            cc.assert_result(prover.check_srs(arr), expect, where, label)
