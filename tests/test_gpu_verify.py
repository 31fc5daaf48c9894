"""GPU tier: the verifier kernels (verify.hip) against the host templates, the big-int pairing model and the expected verdicts of
honest and tampered proofs, on both curves."""
import numpy as np
import pytest

import pairing_model as pmod
import pymodel as pm
from helpers import g1_to_arr, g2_to_arr, mont_to_ints, ints_to_mont, oracle
from verify_cases import identity_ic_case, nonsubgroup_pairs_with_model, oracle_case, tamperings, torsion_pair, wrong_input

import groth16_amd as g
from groth16_amd.serialize import proof_from_bytes, proof_to_bytes
from groth16_amd.verifier import host_verdict

pytestmark = pytest.mark.gpu
NAMES = ["bls12_381", "bn254"]


def as_proof(flat, cp):
    L = cp.fq_limbs64
    return g.Proof(flat[: 2 * L].copy(), flat[2 * L: 6 * L].copy(), flat[6 * L:].copy())


@pytest.fixture(scope="module", params=NAMES)
def setup(request):
    name = request.param
    vk, proofs, x, cp = oracle_case(name)
    with g.Groth16(name, device=0) as prover:
        pvk = prover.prepare_verifying_key(vk)
        yield name, prover, pvk, vk, proofs, x, cp
        pvk.close()


def test_gpu_pairing_equals_host_and_model(setup):
    name, prover, pvk, vk, proofs, x, cp = setup
    G1, G2 = pm.groups(cp)
    pairs = [(G1.mul(cp.g1, 12345), cp.g2), (cp.g1, G2.mul(cp.g2, 777)), (None, cp.g2)]
    g1s, g2s = g1_to_arr([p for p, _ in pairs], cp), g2_to_arr([q for _, q in pairs], cp)
    got = prover.pairing(g1s, g2s)
    assert (got == g.host_pairing(name, g1s, g2s)).all()
    assert (got == pmod.to_ark_limbs(name, pmod.pairing_product(name, pairs))).all()


def test_gpu_pairing_outside_the_subgroups_equals_host_and_model(setup):
    """the plain verifier accepts any on-curve B, so its Miller loop runs on S + T_l (T_l of prime order l in the cofactor), and on
    BLS12-381 on a G1 point outside its subgroup: GPU == host == the big-int model, which never divides by zero there"""
    name, prover, pvk, vk, proofs, x, cp = setup
    for label, pairs, want in nonsubgroup_pairs_with_model(name):
        g1s, g2s = g1_to_arr([p for p, _ in pairs], cp), g2_to_arr([q for _, q in pairs], cp)
        got = prover.pairing(g1s, g2s)
        assert (got == g.host_pairing(name, g1s, g2s)).all(), label
        assert (got == want).all(), label


def pairing_outcome(call):
    """the GT limbs, or the exception's type where the entry point reports a status"""
    try:
        return list(call())
    except g.G16Error as e:
        return type(e)


def test_gpu_pairing_of_a_pure_torsion_point_equals_host(setup):
    """Q = T_l alone (l = 13 on BLS12-381, 10069 on BN254).  On BLS12-381 the loop's chain of multiples reaches a multiple of l: the
    projective T passes through z = 0 and the loop value becomes 0, reported as an unexpected identity.  The big-int model works on
    affine points and defines no value there, so the GPU is held to the host build of the same templates, bit for bit."""
    name, prover, pvk, vk, proofs, x, cp = setup
    l, P, T, hits = torsion_pair(name)
    g1s, g2s = g1_to_arr([P], cp), g2_to_arr([T], cp)
    got = pairing_outcome(lambda: prover.pairing(g1s, g2s))
    assert got == pairing_outcome(lambda: g.host_pairing(name, g1s, g2s))
    if hits:
        assert got is g.UnexpectedIdentity


def test_gpu_cancelling_pairs_and_the_empty_product_give_the_unit(setup):
    name, prover, pvk, vk, proofs, x, cp = setup
    G1, G2 = pm.groups(cp)
    one = pmod.to_ark_limbs(name, pm.Fq12(cp).one)
    P, Q = G1.mul(cp.g1, 0x5EED), G2.mul(cp.g2, 0xF00D)
    for ps, qs in (([P, G1.neg(P)], [Q, Q]), ([P, P], [Q, G2.neg(Q)])):
        g1s, g2s = g1_to_arr(ps, cp), g2_to_arr(qs, cp)
        assert (prover.pairing(g1s, g2s) == one).all()
        assert (g.host_pairing(name, g1s, g2s) == one).all()
    L = cp.fq_limbs64
    assert (prover.pairing(np.zeros((0, 2 * L), np.uint64), np.zeros((0, 4 * L), np.uint64)) == one).all()   # n_pairs = 0


def test_identity_ic(setup):
    """gamma_abc_g1 = [-k G, G] with the public input k: the prepared input is the identity (ic_id in verify_batch_kernel, an
    identity S_IC in the aggregate's tail) and its pair contributes nothing; with k + 1 it is G and the equation fails"""
    name, prover, _, _, _, _, cp = setup
    vk, proofs, x_good, x_bad, cp = identity_ic_case(name)
    n = len(proofs)
    flat = np.stack(proofs)
    pvk = prover.prepare_verifying_key(vk)
    try:
        assert list(prover.verify_verdicts(pvk, flat, [x_good] * n)) == [1] * n
        assert list(prover.verify_verdicts(pvk, flat, [x_bad] * n)) == [0] * n
        assert list(prover.verify_verdicts(pvk, flat, [x_good, x_bad] + [x_good] * (n - 2))) == [1, 0] + [1] * (n - 2)
        for p in proofs:
            assert host_verdict(name, vk, p, x_good) == 1 and host_verdict(name, vk, p, x_bad) == 0
        assert prover.verify_aggregate_verdict(pvk, flat, [x_good] * n) == 1
        assert prover.verify_aggregate_verdict(pvk, flat, [x_bad] * n) == 0
        assert prover.verify_aggregate_verdict(pvk, flat[:1], [x_good]) == 1
        assert prover.verify_aggregate_verdict(pvk, flat[:1], [x_bad]) == 0
        # the same through prepared inputs: an all-zero point is the identity, G is what k + 1 prepares
        L = cp.fq_limbs64
        zero, gen = np.zeros(2 * L, np.uint64), g1_to_arr([cp.g1], cp)[0]
        assert (prover.prepare_inputs(pvk, x_good).reshape(-1) == zero).all() and (prover.prepare_inputs(pvk, x_bad).reshape(-1) == gen).all()
        # and from the device's own preparation (prepare_inputs_tab on the key's resident tables), which the host route above is not
        from groth16_amd import binding
        for xs, want in ((x_good, zero), (x_bad, gen)):
            st, ic = binding.dev_prepare_inputs(g.lib(), prover._ctx.handle, pvk.handle, xs.reshape(1, 1, 4), 1, L)
            assert st == 0 and (ic[0] == want).all()
        from groth16_amd.verifier import verify_batch_prepared
        assert list(verify_batch_prepared(prover._ctx, pvk, flat, np.stack([zero] * n))) == [1] * n
        assert list(verify_batch_prepared(prover._ctx, pvk, flat, np.stack([zero, gen] + [zero] * (n - 2)))) == [1, 0] + [1] * (n - 2)
    finally:
        pvk.close()


def test_alpha_beta_equals_model(setup):
    name, prover, pvk, vk, proofs, x, cp = setup
    from helpers import arr_to_g1, arr_to_g2
    want = pmod.to_ark_limbs(name, pmod.pairing(name, arr_to_g1(vk.alpha_g1, cp)[0], arr_to_g2(vk.beta_g2, cp)[0]))
    assert (pvk.alpha_g1_beta_g2 == want).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_batch_verdicts(setup, n):
    """honest proofs fanned out with rerandomize_proof, tampered and off-curve ones at seeded positions"""
    name, prover, pvk, vk, proofs, x, cp = setup
    base = [as_proof(proofs[0], cp)]
    rng = np.random.default_rng(n)
    for _ in range(3):
        base.append(g.rerandomize_proof(name, vk, base[0]))
    cases = tamperings(proofs, x, cp)
    flat = np.stack([base[i % len(base)].flat() for i in range(n)])
    xs = [x] * n
    want = np.ones(n, dtype=np.uint8)
    pos = rng.choice(n, size=min(n, 2 * len(cases)), replace=False)
    for k, i in enumerate(pos):
        label, p, xi, v = cases[k % len(cases)]
        flat[i], xs[i], want[i] = p, xi, v
    got = prover.verify_verdicts(pvk, flat, xs)
    assert (got == want).all(), np.nonzero(got != want)
    for i in list(pos[:4]) + [0, n - 1]:
        assert host_verdict(name, vk, flat[i], xs[i]) == got[i]
    assert (prover.verify_proofs(pvk, flat, xs) == (want == 1)).all()


def test_identity_a_and_c(setup):
    name, prover, pvk, vk, proofs, x, cp = setup
    L = cp.fq_limbs64
    a0, c0 = proofs[0].copy(), proofs[0].copy()
    a0[: 2 * L] = 0
    c0[6 * L:] = 0
    got = prover.verify_verdicts(pvk, np.stack([a0, c0]), [x, x])
    assert list(got) == [host_verdict(name, vk, a0, x), host_verdict(name, vk, c0, x)] == [0, 0]


def test_no_public_inputs(setup):
    """a key with gamma_abc_g1 = [IC] verifies the same proof with no inputs (l = 0)"""
    name, prover, pvk, vk, proofs, x, cp = setup
    ic = prover.prepare_inputs(pvk, x)
    vk0 = g.VerifyingKey(name, vk.alpha_g1, vk.beta_g2, vk.gamma_g2, vk.delta_g2, ic.reshape(1, -1))
    pvk0 = prover.prepare_verifying_key(vk0)
    try:
        assert prover.verify_proof(pvk0, as_proof(proofs[0], cp), [])
        assert list(prover.verify_verdicts(pvk0, np.stack(proofs), [[], []])) == [1, 1]
        assert g.verify_proof_host(name, vk0, proofs[0], [])
        with pytest.raises(g.MalformedVerifyingKey):
            prover.verify_proof(pvk0, as_proof(proofs[0], cp), x)
    finally:
        pvk0.close()


def test_r_s_zero_proofs(setup):
    name, prover, pvk, vk, proofs, x, cp = setup
    orc = oracle()
    ck = orc.syn_circuit(name, 4, 9)
    pk, _ = orc.setup(ck, 3)
    zero = np.zeros(4, dtype=np.uint64)
    flat, _ = orc.prove(pk, ck, zero, zero)
    assert prover.verify_proof(pvk, as_proof(np.asarray(flat, np.uint64), cp), x)


def test_proofs_read_back_from_bytes(setup):
    name, prover, pvk, vk, proofs, x, cp = setup
    for compressed in (True, False):
        p = proof_from_bytes(name, proof_to_bytes(name, as_proof(proofs[1], cp), compressed), compressed)
        assert prover.verify_proof(pvk, p, x)


def test_prepared_inputs_equal_verify_proof(setup):
    name, prover, pvk, vk, proofs, x, cp = setup
    for p in proofs:
        pr = as_proof(p, cp)
        for xi in (x, wrong_input(x, cp)):
            ic = prover.prepare_inputs(pvk, xi)
            assert prover.verify_proof_with_prepared_inputs(pvk, pr, ic) == prover.verify_proof(pvk, pr, xi)
    with pytest.raises(g.MalformedVerifyingKey):
        prover.verify_proof(pvk, as_proof(proofs[0], cp), np.concatenate([x, x]))


def test_multi_device_context_keeps_input_order(setup):
    name, _, _, vk, proofs, x, cp = setup
    cases = tamperings(proofs, x, cp)
    flat = np.stack([c[1] for c in cases] * 5)
    xs = [c[2] for c in cases] * 5
    want = np.array([c[3] for c in cases] * 5, dtype=np.uint8)
    with g.Groth16(name, device=[0, 0]) as multi:
        pvk = multi.prepare_verifying_key(vk)
        try:
            assert (multi.verify_verdicts(pvk, flat, xs) == want).all()
            for label, p, xi, v in (cases[0], cases[3]):   # n = 1: the first of the two chunks is empty
                assert list(multi.verify_verdicts(pvk, p[None], [xi])) == [host_verdict(name, vk, p, xi)] == [v], label
        finally:
            pvk.close()


def test_gpu_made_proof_is_accepted(setup):
    """a proof of the GPU prover (syn circuit, as smoke() makes it) and its rerandomisations"""
    name, prover, pvk, vk, proofs, x, cp = setup
    orc = oracle()
    ck = orc.syn_circuit(name, 10, 1)
    pk, ex = orc.setup(ck, 5)
    mats = g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints, *[(m.row_ptr, m.col, m.val) for m in ck.abc])
    gpk = g.ProvingKey(name, pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, pk.a_query, pk.b_g1_query, pk.b_g2_query,
                       pk.h_query, pk.l_query, ex["gamma_g2"].reshape(1, -1), np.ascontiguousarray(ex["gamma_abc"]))
    r, s = orc.rand_fr(name, 11, 1)[0], orc.rand_fr(name, 12, 1)[0]
    proof = prover.create_proof_with_reduction_and_matrices(gpk, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z)
    pvk2 = prover.prepare_verifying_key(gpk)   # a ProvingKey that carries gamma_g2 / gamma_abc_g1
    try:
        xi = np.ascontiguousarray(ck.z[1: ck.num_inputs]).reshape(-1, 4)
        batch = [proof] + [g.rerandomize_proof(name, gpk, proof) for _ in range(3)]
        assert prover.verify_proofs(pvk2, batch, [xi] * 4).all()
        if len(xi):
            assert not prover.verify_proof(pvk2, proof, ints_to_mont([(mont_to_ints(xi, cp.r)[0] + 1) % cp.r] +
                                                                     mont_to_ints(xi, cp.r)[1:], cp.r, 4))
    finally:
        pvk2.close()


@pytest.mark.parametrize("curve", NAMES)
def test_2_20_gpu_proof_with_gpu_key_is_accepted(curve):
    """a 2^20-constraint proof of the GPU prover under a key made by the GPU generator (which fills gamma_g2 / gamma_abc_g1)"""
    cp = pm.CURVES[curve]
    orc = oracle()
    ck = orc.syn_circuit(curve, 20, 37)
    toxic = orc.rand_fr(curve, 920, 5)                           # alpha beta gamma delta t
    gens = orc.setup(orc.syn_circuit(curve, 2, 1), 3)[1]
    r, s = orc.rand_fr(curve, 71, 1)[0], orc.rand_fr(curve, 72, 1)[0]
    with g.Groth16(curve, device=0) as prover:
        mats = g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints,
                                    *[(m.row_ptr, m.col, m.val) for m in ck.abc])
        pk = prover.generate_parameters_with_qap(mats, toxic[0], toxic[1], toxic[2], toxic[3], gens["g1gen"], gens["g2gen"], toxic[4])
        proof = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z)
        pvk = prover.prepare_verifying_key(pk)
        try:
            xi = np.ascontiguousarray(ck.z[1: ck.num_inputs]).reshape(-1, 4)
            assert prover.verify_proof(pvk, proof, xi)
            assert g.verify_proof_host(curve, pk, proof, xi)
            if len(xi):
                assert not prover.verify_proof(pvk, proof, wrong_input(xi, cp))
        finally:
            pvk.close()
