"""GPU tier: the membership kernels (verify_subgroup.hip) against the host twin and the big-int model's flags, per point, per proof
and inside the checked aggregate verifier, on both curves."""
import ctypes as C

import numpy as np
import pytest

import pymodel as pm
from aggregate_cases import coeffs_for, honest_base
from helpers import arr_to_g1, arr_to_g2, g1_to_arr, g2_to_arr
from subgroup_cases import NAMES, case_arrays, cases, model_groups
from verify_cases import oracle_case, wrong_input

import groth16_amd as g
from groth16_amd.binding import ptr64
from groth16_amd.verifier import host_aggregate_verdict

pytestmark = pytest.mark.gpu
N_PROOFS = 67


@pytest.fixture(scope="module", params=NAMES)
def setup(request):
    name = request.param
    vk, proofs, x, cp = oracle_case(name)
    base = honest_base(name, vk, proofs, cp)
    honest = np.stack([base[i % len(base)] for i in range(N_PROOFS)])
    with g.Groth16(name, device=0) as prover:
        pvk = prover.prepare_verifying_key(vk)
        yield name, prover, pvk, vk, x, cp, honest
        pvk.close()


def plus_torsion(flat, which, cp, name, l=None):
    """the proof with A / B / C (which = 0 / 1 / 2) replaced by itself + T, T of prime order l (the smallest by default) outside the
    subgroup: on its curve, honest subgroup part"""
    L = cp.fq_limbs64
    g2 = which == 1
    G = model_groups(cp)[g2]
    _, torsion = cases(name, g2)
    T = torsion[l if l else min(torsion)]
    lo, hi = ((0, 2 * L), (2 * L, 6 * L), (6 * L, 8 * L))[which]
    P = (arr_to_g2 if g2 else arr_to_g1)(flat[lo:hi], cp)[0]
    out = flat.copy()
    out[lo:hi] = (g2_to_arr if g2 else g1_to_arr)([G.add(P, T)], cp)[0]
    return out


def off_curve(flat, which, cp, name):
    L = cp.fq_limbs64
    g2 = which == 1
    labels, pts, _ = case_arrays(name, g2)
    lo, hi = ((0, 2 * L), (2 * L, 6 * L), (6 * L, 8 * L))[which]
    out = flat.copy()
    out[lo:hi] = pts[labels.index("off_curve")]
    return out


def tampered_batch(name, cp, honest):
    """(batch, flags): S + T in A, B, C of three proofs, an off-curve C, and a proof that is off a subgroup AND off a curve (2 wins).
    BN254's G1 is the whole curve (cofactor 1): there only B can leave its subgroup, so proofs 3 and 40 stay honest and the last
    proof pairs B + T with an off-curve C"""
    flat, want = honest.copy(), np.ones(N_PROOFS, dtype=np.uint8)
    bls = name == "bls12_381"
    if bls:
        flat[3], want[3] = plus_torsion(flat[3], 0, cp, name), 0
        flat[40], want[40] = plus_torsion(flat[40], 2, cp, name, 11), 0
    flat[20], want[20] = plus_torsion(flat[20], 1, cp, name), 0
    flat[50], want[50] = off_curve(flat[50], 2, cp, name), 2
    if bls:
        flat[66] = off_curve(plus_torsion(flat[66], 0, cp, name, 10177), 1, cp, name)
    else:
        flat[66] = off_curve(plus_torsion(flat[66], 1, cp, name), 2, cp, name)
    want[66] = 2
    return flat, want


@pytest.mark.parametrize("g2", [False, True])
def test_points_equal_the_host_twin(setup, g2):
    """the whole case list tiled to 130 points: two full waves and a 2-lane tail"""
    name, prover = setup[0], setup[1]
    _, pts, want = case_arrays(name, g2)
    idx = np.arange(130) % len(want)
    tiled = np.ascontiguousarray(pts[idx])
    got = prover.check_subgroups(tiled, g2)
    print(name, "g2" if g2 else "g1", "device flags", got[: len(want)].tolist(), "model", want.tolist())
    assert got.tobytes() == g.check_subgroups_host(name, tiled, g2).tobytes()
    assert (got == want[idx]).all()
    assert prover.check_subgroups(tiled[:0], g2).shape == (0,)


def test_proof_flags(setup):
    name, prover, pvk, vk, x, cp, honest = setup
    flat, want = tampered_batch(name, cp, honest)
    assert (prover.check_proof_subgroups(honest) == 1).all()
    got = prover.check_proof_subgroups(flat)
    print(name, "proof flags", got.tolist())
    assert (got == want).all()
    assert prover.check_proof_subgroups(flat[:0]).shape == (0,)
    with g.Groth16(name, device=[0, 0]) as multi:   # two chunks: the order survives the split
        assert (multi.check_proof_subgroups(flat) == want).all()
        _, pts, flags = case_arrays(name, True)
        assert (multi.check_subgroups(pts, True) == flags).all()
        # n = 1: the first of the two chunks is empty.  One honest and one tampered item, against the host twin
        L = cp.fq_limbs64
        for i in (0, 20):
            a, b, c = (g.check_subgroups_host(name, flat[i, lo:hi].reshape(1, -1), g2)[0]
                       for lo, hi, g2 in ((0, 2 * L, False), (2 * L, 6 * L, True), (6 * L, 8 * L, False)))
            host = 2 if 2 in (a, b, c) else min(a, b, c)
            assert list(multi.check_proof_subgroups(flat[i: i + 1])) == [host] == [want[i]]
        for i in (int(np.argmax(flags == 1)), int(np.argmax(flags == 0))):
            assert list(multi.check_subgroups(pts[i: i + 1], True)) == list(g.check_subgroups_host(name, pts[i: i + 1], True)) == [flags[i]]


def direct_aggregate(prover, pvk, flat, xs, coeffs):
    """g16_verify_aggregate called through ctypes, as before this feature"""
    n = flat.shape[0]
    xw = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.uint64).reshape(-1) for v in xs]))
    r = np.array([[c & (2**64 - 1), c >> 64] for c in coeffs], dtype=np.uint64)
    v = np.zeros(1, dtype=np.uint8)
    lb = g.lib()
    lb.check(lb.c.g16_verify_aggregate(prover._ctx.handle, pvk.handle, ptr64(np.ascontiguousarray(flat).reshape(-1)), n, ptr64(xw), xw.size // (4 * n),
                                       ptr64(r.reshape(-1)), v.ctypes.data_as(C.c_void_p)))
    return int(v[0])


def test_checked_aggregate_verdicts(setup):
    name, prover, pvk, vk, x, cp, honest = setup
    xs = [x] * N_PROOFS
    coeffs = coeffs_for(N_PROOFS, 11)
    bls = name == "bls12_381"
    outside = honest.copy()
    outside[31] = plus_torsion(outside[31], 0, cp, name, 3) if bls else plus_torsion(outside[31], 1, cp, name, 10069)
    both = outside.copy()
    both[5] = off_curve(both[5], 0, cp, name)
    bad_x = list(xs)
    bad_x[66] = wrong_input(x, cp)
    for flat, xt, want in ((honest, xs, 1), (outside, xs, 3), (both, xs, 2), (honest, bad_x, 0)):
        for r in (coeffs, None):
            assert prover.verify_aggregate_verdict(pvk, flat, xt, r, check_subgroups=True) == want
        assert prover.verify_proofs_aggregate(pvk, flat, xt, coeffs, check_subgroups=True) == (want == 1)
        # unchecked: today's verdicts, whatever they are for a batch outside the soundness condition
        today = direct_aggregate(prover, pvk, flat, xt, coeffs)
        assert today in (0, 1, 2) and (today == want or want == 3)
        assert prover.verify_aggregate_verdict(pvk, flat, xt, coeffs, check_subgroups=False) == today
        assert prover.verify_aggregate_verdict(pvk, flat, xt, coeffs) == today
    with g.Groth16(name, device=[0, 0]) as multi:   # each device checks its own chunk
        pvk2 = multi.prepare_verifying_key(vk)
        try:
            for flat, xt, want in ((honest, xs, 1), (outside, xs, 3), (both, xs, 2), (honest, bad_x, 0)):
                assert multi.verify_aggregate_verdict(pvk2, flat, xt, coeffs, check_subgroups=True) == want
            # n = 1: the first of the two chunks is empty.  The host form has no membership stage: it answers for members only
            for flat, xt, want in ((honest[:1], xs[:1], 1), (honest[66:], bad_x[66:], 0)):
                assert multi.verify_aggregate_verdict(pvk2, flat, xt, coeffs[:1], check_subgroups=True) == want
                assert host_aggregate_verdict(name, vk, flat, xt, coeffs[:1]) == want
            assert multi.verify_aggregate_verdict(pvk2, outside[31:32], xs[:1], coeffs[:1], check_subgroups=True) == 3
        finally:
            pvk2.close()


def test_or_each_names_the_tampered_proofs(setup):
    name, prover, pvk, vk, x, cp, honest = setup
    flat, flags = tampered_batch(name, cp, honest)
    xs = [x] * N_PROOFS
    xs[10] = wrong_input(x, cp)
    want = flags == 1
    want[10] = False
    got = prover.verify_proofs_aggregate_or_each(pvk, flat, xs, check_subgroups=True)
    assert got.dtype == bool and (got == want).all()
    assert prover.verify_proofs_aggregate_or_each(pvk, honest, [x] * N_PROOFS, check_subgroups=True).all()
