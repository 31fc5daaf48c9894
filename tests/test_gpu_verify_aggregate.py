"""GPU tier: g16_verify_aggregate (verify_aggregate.hip) against the per-proof verdicts, the host form on the same coefficients,
the cancelling pair across workgroups, many public inputs and a two-chunk context, on both curves."""
import random

import numpy as np
import pytest

import pymodel as pm
from aggregate_cases import as_proof, cancelling_pair, coeffs_for, expected_verdict
from helpers import arr_to_g1, g1_to_arr, ints_to_mont, mont_to_ints
from verify_cases import oracle_case, tamperings

import groth16_amd as g
from groth16_amd.verifier import host_aggregate_verdict, host_verdict

pytestmark = pytest.mark.gpu
NAMES = ["bls12_381", "bn254"]


@pytest.fixture(scope="module", params=NAMES)
def setup(request):
    name = request.param
    vk, proofs, x, cp = oracle_case(name)
    base = [as_proof(proofs[0], cp)]
    for _ in range(3):
        base.append(g.rerandomize_proof(name, vk, base[0]))
    with g.Groth16(name, device=0) as prover:
        pvk = prover.prepare_verifying_key(vk)
        yield name, prover, pvk, vk, proofs, x, cp, [b.flat() for b in base]
        pvk.close()


def fan_out(base, n):
    return np.stack([base[i % len(base)] for i in range(n)])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_aggregate_verdicts(setup, n):
    """batches built as test_gpu_verify.test_batch_verdicts builds them"""
    name, prover, pvk, vk, proofs, x, cp, base = setup
    rng = np.random.default_rng(n)
    cases = tamperings(proofs, x, cp)
    honest = fan_out(base, n)
    xs = [x] * n
    coeffs = coeffs_for(n, n)
    assert prover.verify_aggregate_verdict(pvk, honest, xs, coeffs) == 1
    assert prover.verify_aggregate_verdict(pvk, honest, xs) == 1
    assert prover.verify_proofs_aggregate(pvk, honest, xs)
    # the whole tampered set (off-curve points among it), then only the tamperings that stay on the curves
    for keep in (cases, [c for c in cases if c[3] != 2]):
        flat, xt, want = honest.copy(), list(xs), np.ones(n, dtype=np.uint8)
        pos = rng.choice(n, size=min(n, 2 * len(keep)), replace=False)
        for k, i in enumerate(pos):
            label, p, xi, v = keep[k % len(keep)]
            flat[i], xt[i], want[i] = p, xi, v
        rule = expected_verdict(want)
        assert (prover.verify_verdicts(pvk, flat, xt) == want).all()
        assert prover.verify_aggregate_verdict(pvk, flat, xt, coeffs) == rule
        assert prover.verify_aggregate_verdict(pvk, flat, xt) == rule
        if n <= 65:
            assert host_aggregate_verdict(name, vk, flat, xt, coeffs) == rule
    if n <= 65:
        assert host_aggregate_verdict(name, vk, honest, xs, coeffs) == 1


def test_one_bad_proof_at_each_end(setup):
    """a single invalid proof in the first / last lane of a batch that is not a multiple of the workgroup"""
    name, prover, pvk, vk, proofs, x, cp, base = setup
    bad = tamperings(proofs, x, cp)[3][1]   # c_is_a
    for n in (130, 1000):
        for i in (0, n - 1, n // 2):
            flat = fan_out(base, n)
            flat[i] = bad
            assert prover.verify_aggregate_verdict(pvk, flat, [x] * n, coeffs_for(n, i + 1)) == 0


def test_cancelling_pair_across_workgroups(setup):
    """positions 0 and n - 1 of n = 1000: the cross-workgroup reduction carries both halves of the attack"""
    name, prover, pvk, vk, proofs, x, cp, base = setup
    n = 1000
    p2, q2 = cancelling_pair(proofs[0], proofs[1], cp)
    assert host_verdict(name, vk, p2, x) == 0 and host_verdict(name, vk, q2, x) == 0
    flat = fan_out(base, n)
    flat[0], flat[n - 1] = p2, q2
    xs = [x] * n
    got = prover.verify_verdicts(pvk, flat, xs)
    assert got[0] == 0 and got[n - 1] == 0 and (got[1: n - 1] == 1).all()
    assert prover.verify_aggregate_verdict(pvk, flat, xs, [1] * n) == 1      # the plain product accepts: the attack
    assert prover.verify_aggregate_verdict(pvk, flat, xs, [1] * (n - 1) + [2]) == 0
    assert prover.verify_aggregate_verdict(pvk, flat, xs, coeffs_for(n, 3)) == 0
    assert prover.verify_aggregate_verdict(pvk, flat, xs) == 0


def test_edges(setup):
    name, prover, pvk, vk, proofs, x, cp, base = setup
    L = cp.fq_limbs64
    assert prover.verify_aggregate_verdict(pvk, np.zeros((0, 8 * L), np.uint64), []) == 1
    for label, proof, xi, want in tamperings(proofs, x, cp):
        assert prover.verify_aggregate_verdict(pvk, [proof], [xi], [0x1234567]) == want, label
    with pytest.raises(g.G16Error) as err:
        prover.verify_aggregate_verdict(pvk, np.stack(proofs), [x, x], [5, 0])
    assert err.value.status == 3
    with pytest.raises(g.MalformedVerifyingKey):
        prover.verify_aggregate_verdict(pvk, np.stack(proofs), [np.concatenate([x, x[:1]])] * 2)
    a0, c0 = proofs[0].copy(), proofs[0].copy()
    a0[: 2 * L] = 0
    c0[6 * L:] = 0
    for bad in (a0, c0):
        assert prover.verify_aggregate_verdict(pvk, np.stack([proofs[1], bad]), [x, x], [7, 9]) == 0
        assert prover.verify_aggregate_verdict(pvk, [bad], [x]) == 0


def wide_key(name, vk, x, cp, n_inputs, n_vectors, seed):
    """A key with n_inputs public inputs under which the case's proofs still verify: gamma_abc'[j] = k_j G for j >= 1, and every
    input vector x' has sum_j x'_j k_j = c, with gamma_abc'[0] = IC - c G (IC: the prepared input of the original key)."""
    G1, _ = pm.groups(cp)
    rng = random.Random(seed)
    gabc = arr_to_g1(vk.gamma_abc_g1, cp)
    ic = gabc[0]
    for v, b in zip(mont_to_ints(x.reshape(-1, 4), cp.r), gabc[1:]):
        ic = G1.add(ic, G1.mul(b, v))
    ks = [rng.randrange(1, cp.r) for _ in range(n_inputs)]
    c = rng.randrange(cp.r)
    new = [G1.add(ic, G1.neg(G1.mul(cp.g1, c)))] + [G1.mul(cp.g1, k) for k in ks]
    vectors = []
    for _ in range(n_vectors):
        v = [rng.randrange(cp.r) for _ in range(n_inputs - 1)]
        rest = (c - sum(a * k for a, k in zip(v, ks))) % cp.r
        v.append(rest * pow(ks[-1], -1, cp.r) % cp.r)
        vectors.append(ints_to_mont(v, cp.r, 4).reshape(-1, 4))
    return g.VerifyingKey(name, vk.alpha_g1, vk.beta_g2, vk.gamma_g2, vk.delta_g2, g1_to_arr(new, cp)), vectors


def test_sixteen_public_inputs(setup):
    """every column of the t_j reduction carries its own values: a different input vector per proof"""
    name, prover, pvk, vk, proofs, x, cp, base = setup
    n = 300
    vk16, vectors = wide_key(name, vk, x, cp, 16, 7, seed=21)
    pvk16 = prover.prepare_verifying_key(vk16)
    try:
        flat = fan_out(base, n)
        xs = [vectors[i % len(vectors)] for i in range(n)]
        assert (prover.verify_verdicts(pvk16, flat, xs) == 1).all()
        assert prover.verify_aggregate_verdict(pvk16, flat, xs, coeffs_for(n, 16)) == 1
        assert prover.verify_aggregate_verdict(pvk16, flat, xs) == 1
        assert host_aggregate_verdict(name, vk16, flat[:9], xs[:9], coeffs_for(9, 2)) == 1
        for col in (0, 7, 15):
            bad = list(xs)
            v = mont_to_ints(bad[211], cp.r)
            v[col] = (v[col] + 1) % cp.r
            bad[211] = ints_to_mont(v, cp.r, 4).reshape(-1, 4)
            assert prover.verify_aggregate_verdict(pvk16, flat, bad, coeffs_for(n, 16)) == 0
            assert prover.verify_aggregate_verdict(pvk16, flat, bad) == 0
    finally:
        pvk16.close()


def test_two_chunk_context_and_or_each(setup):
    name, prover, pvk, vk, proofs, x, cp, base = setup
    n = 333
    cases = tamperings(proofs, x, cp)
    honest = fan_out(base, n)
    two_bad, xt = honest.copy(), [x] * n
    two_bad[5], two_bad[n - 2] = cases[3][1], cases[4][1]
    off = honest.copy()
    off[n - 1] = cases[6][1]
    p2, q2 = cancelling_pair(proofs[0], proofs[1], cp)
    cancel = honest.copy()
    cancel[0], cancel[n - 1] = p2, q2            # one half in each device's chunk
    coeffs = coeffs_for(n, 8)
    want = prover.verify_proofs(pvk, two_bad, xt)
    assert list(np.nonzero(~want)[0]) == [5, n - 2]
    assert (prover.verify_proofs_aggregate_or_each(pvk, two_bad, xt) == want).all()
    assert prover.verify_proofs_aggregate_or_each(pvk, honest, xt).all()
    with g.Groth16(name, device=[0, 0]) as multi:
        pvk2 = multi.prepare_verifying_key(vk)
        try:
            # verdicts with (seeded coefficients, all ones, the library's own draw)
            for flat, verdicts in ((honest, (1, 1, 1)), (two_bad, (0, 0, 0)), (off, (2, 2, 2)), (cancel, (0, 1, 0))):
                for r, v in zip((coeffs, [1] * n, None), verdicts):
                    assert prover.verify_aggregate_verdict(pvk, flat, xt, r) == v
                    assert multi.verify_aggregate_verdict(pvk2, flat, xt, r) == v
            assert (multi.verify_proofs_aggregate_or_each(pvk2, two_bad, xt) == want).all()
            for label, p, xi, v in (cases[0], cases[3]):   # n = 1: the first of the two chunks is empty
                assert multi.verify_aggregate_verdict(pvk2, p[None], [xi], coeffs[:1]) == v, label
                assert host_aggregate_verdict(name, vk, p[None], [xi], coeffs[:1]) == v, label
        finally:
            pvk2.close()


@pytest.mark.parametrize("n", [2**18 + 77])
def test_proofs_sharing_a_lane(setup, n):
    """past twice the resident lanes of the device, two or more proofs share a lane and its accumulator"""
    name, prover, pvk, vk, proofs, x, cp, base = setup
    L = cp.fq_limbs64
    idx = np.arange(n) % len(base)
    honest = np.ascontiguousarray(np.stack(base)[idx])
    xs = np.ascontiguousarray(np.broadcast_to(x.reshape(1, -1, 4), (n,) + x.reshape(-1, 4).shape))
    coeffs = np.random.default_rng(7).integers(1, 2**63, size=(n, 2)).astype(np.uint64)
    ones = np.tile(np.array([[1, 0]], dtype=np.uint64), (n, 1))
    assert prover.verify_aggregate_verdict(pvk, honest, xs, coeffs) == 1
    assert prover.verify_aggregate_verdict(pvk, honest, xs) == 1
    bad = tamperings(proofs, x, cp)[3][1]
    for i in (1, n // 2, n - 1):
        flat = honest.copy()
        flat[i] = bad
        assert prover.verify_aggregate_verdict(pvk, flat, xs, coeffs) == 0
    p2, q2 = cancelling_pair(proofs[0], proofs[1], cp)
    for i, j in ((0, 1), (2, n - 1)):   # neighbours (one lane when two proofs share it), and far apart
        flat = honest.copy()
        flat[i], flat[j] = p2, q2
        assert prover.verify_aggregate_verdict(pvk, flat, xs, ones) == 1
        assert prover.verify_aggregate_verdict(pvk, flat, xs, coeffs) == 0
    off = honest.copy()
    off[n - 3, 2 * L - 1] ^= np.uint64(1) << np.uint64(20)
    assert prover.verify_aggregate_verdict(pvk, off, xs, coeffs) == 2
