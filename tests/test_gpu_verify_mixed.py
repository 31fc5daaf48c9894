"""GPU tier: g16_verify_aggregate_mixed (verify_mixed.hip) on batches that interleave up to 65 verifying keys, on both curves:
against the per-key verify_verdicts, the host form on the same coefficients, the single-key call, and the attacks that tell a
per-key sum of r_i C_i from a global one.  The per-proof stage of this path puts one proof in a lane (no lane sharing), so there is
no large shape for it here."""
import numpy as np
import pytest

import pymodel as pm
from aggregate_cases import cancelling_pair, coeffs_for, expected_verdict
from mixed_key_cases import NAMES, batch, mixed_keys, positions_of
from subgroup_cases import cases as subgroup_cases, to_arr
from verify_cases import tamperings

import groth16_amd as g
from groth16_amd.verifier import host_aggregate_mixed_verdict

pytestmark = pytest.mark.gpu
KS = [1, 2, 3, 64, 65]   # 64 and 65 cross the wave of the per-key stage
ORDERS = ["grouped", "round_robin", "shuffled"]


def sizes_for(K):
    """runs of equal keys that begin and end inside, at and across the 64-lane boundaries of the grouped order (n <= 400)"""
    if K == 1:
        return [130]
    if K == 2:
        return [63, 66]
    head = [1, 63, 1, 64, 65, 2]   # runs [0,1) [1,64) [64,65) [65,129) [129,194) [194,196)
    return (head + [i % 3 + 1 for i in range(K)])[:K]


@pytest.fixture(scope="module", params=NAMES)
def setup(request):
    name = request.param
    keys = mixed_keys(name, 65)
    with g.Groth16(name, device=0) as prover:
        pvks = [prover.prepare_verifying_key(c.vk) for c in keys]
        yield name, prover, keys, pvks, pm.CURVES[name]
        for p in pvks:
            p.close()


def per_key_verdicts(prover, pvks, key_of, flat, xs):
    """what the parent offers: verify_verdicts once per key, put back in input order"""
    out = np.zeros(len(key_of), dtype=np.uint8)
    for k in np.unique(key_of):
        idx = positions_of(key_of, k)
        out[idx] = prover.verify_verdicts(pvks[k], flat[idx], [xs[i] for i in idx])
    return out


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("K", KS)
def test_honest_batches(setup, K, order):
    name, prover, keys, pvks, cp = setup
    flat, key_of, xs = batch(keys[:K], sizes_for(K), order, seed=K)
    n = len(key_of)
    assert n <= 400
    assert prover.verify_aggregate_mixed_verdict(pvks[:K], key_of, flat, xs, coeffs_for(n, K)) == 1
    assert prover.verify_aggregate_mixed_verdict(pvks[:K], key_of, flat, xs) == 1
    assert prover.verify_proofs_aggregate_mixed(pvks[:K], key_of, flat, xs)


@pytest.mark.parametrize("on_curve_only", [False, True], ids=["all", "on_curve"])
@pytest.mark.parametrize("K", KS)
def test_tamperings_scattered_over_the_keys(setup, K, on_curve_only):
    """the whole tampered set (off-curve points among it), and only the tamperings that stay on the curves"""
    name, prover, keys, pvks, cp = setup
    flat0, key_of, xs0 = batch(keys[:K], sizes_for(K), "shuffled", seed=100 + K)
    n = len(key_of)
    rng = np.random.default_rng(2 * K + on_curve_only)
    coeffs = coeffs_for(n, 7 * K)
    with_inputs = [k for k in range(K) if keys[k].num_public]
    flat, xt, want = flat0.copy(), list(xs0), np.ones(n, dtype=np.uint8)
    for k in rng.choice(with_inputs, size=min(len(with_inputs), 6), replace=False):
        cases = [c for c in tamperings(keys[k].proofs, keys[k].vectors[0], cp) if c[3] != 1 and not (on_curve_only and c[3] == 2)]
        label, p, xi, v = cases[int(rng.integers(len(cases)))]
        i = int(rng.choice(positions_of(key_of, k)))
        flat[i], xt[i], want[i] = p, xi, v
    assert (per_key_verdicts(prover, pvks, key_of, flat, xt) == want).all()
    rule = expected_verdict(want)
    assert rule in ((0,) if on_curve_only else (0, 2))
    assert prover.verify_aggregate_mixed_verdict(pvks[:K], key_of, flat, xt, coeffs) == rule
    assert prover.verify_aggregate_mixed_verdict(pvks[:K], key_of, flat, xt) == rule


def test_small_batches_equal_the_host_form(setup):
    name, prover, keys, pvks, cp = setup
    picks = [1, 3, 5, 6]   # 0, 3 and 16 public inputs beside an oracle key
    sub, sub_pvks = [keys[k] for k in picks], [pvks[k] for k in picks]
    vks = [c.vk for c in sub]
    flat, key_of, xs = batch(sub, [20, 11, 30, 4], "round_robin")
    n = len(key_of)
    assert n == 65
    coeffs = coeffs_for(n, 12)
    assert prover.verify_aggregate_mixed_verdict(sub_pvks, key_of, flat, xs, coeffs) == 1
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xs, coeffs) == 1
    for label, p, xi, want in tamperings(sub[2].proofs, sub[2].vectors[0], cp)[2:]:
        bad, xt = flat.copy(), list(xs)
        i = positions_of(key_of, 2)[-1]
        bad[i], xt[i] = p, xi
        got = prover.verify_aggregate_mixed_verdict(sub_pvks, key_of, bad, xt, coeffs)
        assert got == host_aggregate_mixed_verdict(name, vks, key_of, bad, xt, coeffs) == want, label


def test_one_key_equals_the_single_key_call(setup):
    name, prover, keys, pvks, cp = setup
    flat, key_of, xs = batch(keys[:1], [130])
    coeffs = coeffs_for(130, 5)
    for label, p, xi, want in tamperings(keys[0].proofs, keys[0].vectors[0], cp):
        bad, xt = flat.copy(), list(xs)
        bad[77], xt[77] = p, xi
        for r in (coeffs, [1] * 130):
            assert prover.verify_aggregate_mixed_verdict(pvks[:1], key_of, bad, xt, r) == prover.verify_aggregate_verdict(pvks[0], bad, xt, r) == want, label


def test_a_proof_under_the_wrong_key_is_rejected(setup):
    name, prover, keys, pvks, cp = setup
    flat, key_of, xs = batch(keys[:3], [70, 3, 60], "shuffled", seed=4)   # equal input counts, three trapdoors
    coeffs = coeffs_for(len(key_of), 2)
    assert prover.verify_aggregate_mixed_verdict(pvks[:3], key_of, flat, xs, coeffs) == 1
    for i in (0, 64, len(key_of) - 1):
        wrong = key_of.copy()
        wrong[i] = (wrong[i] + 1) % 3
        assert prover.verify_aggregate_mixed_verdict(pvks[:3], wrong, flat, xs, coeffs) == 0
        assert prover.verify_aggregate_mixed_verdict(pvks[:3], wrong, flat, xs) == 0


def test_sums_are_per_key(setup):
    """cancelling_pair (C + D, C - D) at positions 0 and n - 1, other keys' proofs between them in input order.  Under ONE key
    both halves reach the same S_C_k and the plain product (coefficients all 1) accepts -- what a segmented sum must do; under two
    DIFFERENT keys D and -D meet different deltas and even the plain product rejects"""
    name, prover, keys, pvks, cp = setup
    x = keys[0].vectors[0]
    mid, mid_keys, mid_xs = batch(keys[:5], [0, 70, 64, 3, 61], "shuffled", seed=8)
    n = len(mid_keys) + 2
    p2, q2 = cancelling_pair(keys[0].proofs[0], keys[0].proofs[1], cp)
    flat = np.concatenate([p2[None], mid, q2[None]])
    key_of = np.concatenate([[0], mid_keys, [0]]).astype(np.uint32)
    xs = [x] + mid_xs + [x]
    got = per_key_verdicts(prover, pvks, key_of, flat, xs)
    assert got[0] == 0 and got[n - 1] == 0 and (got[1: n - 1] == 1).all()
    assert prover.verify_aggregate_mixed_verdict(pvks[:5], key_of, flat, xs, [1] * n) == 1
    assert prover.verify_aggregate_mixed_verdict(pvks[:5], key_of, flat, xs, [1] * (n - 1) + [2]) == 0
    assert prover.verify_aggregate_mixed_verdict(pvks[:5], key_of, flat, xs, coeffs_for(n, 3)) == 0
    assert prover.verify_aggregate_mixed_verdict(pvks[:5], key_of, flat, xs) == 0
    # the second half under key 7, a derived copy of key 0
    assert keys[7].num_public == keys[0].num_public
    p3, q3 = cancelling_pair(keys[0].proofs[0], keys[7].proofs[1], cp)
    flat[0], flat[n - 1] = p3, q3
    key_of[n - 1] = 7
    assert prover.verify_aggregate_mixed_verdict(pvks[:8], key_of, flat, xs, [1] * n) == 0


def test_edges(setup):
    name, prover, keys, pvks, cp = setup
    L = cp.fq_limbs64
    assert [keys[k].num_public for k in (3, 6)] == [0, 16]
    assert prover.verify_aggregate_mixed_verdict(pvks[:3], [], np.zeros((0, 8 * L), np.uint64), []) == 1
    assert prover.verify_aggregate_mixed_verdict([], [], np.zeros((0, 8 * L), np.uint64), []) == 1
    # keys 1, 4 and 5 have no proof; 0 public inputs next to 16
    flat, key_of, xs = batch(keys[:7], [2, 0, 1, 5, 0, 0, 9], "shuffled", seed=1)
    n = len(key_of)
    coeffs = coeffs_for(n, 31)
    assert prover.verify_aggregate_mixed_verdict(pvks[:7], key_of, flat, xs, coeffs) == 1
    bad = list(xs)
    i = positions_of(key_of, 6)[3]
    bad[i] = bad[i].copy()
    bad[i][15, 0] ^= np.uint64(1)
    assert prover.verify_aggregate_mixed_verdict(pvks[:7], key_of, flat, bad, coeffs) == 0
    # the same handle under two indices
    twice = key_of.copy()
    twice[positions_of(key_of, 6)[::2]] = 7
    assert prover.verify_aggregate_mixed_verdict(pvks[:7] + [pvks[6]], twice, flat, xs, coeffs) == 1
    assert prover.verify_aggregate_mixed_verdict(pvks[:7] + [pvks[6]], twice, flat, bad, coeffs) == 0
    # membership: every point of an honest proof is a member; B replaced by a curve point outside the subgroup gives 3
    assert prover.verify_aggregate_mixed_verdict(pvks[:7], key_of, flat, xs, coeffs, check_subgroups=True) == 1
    assert prover.verify_aggregate_mixed_verdict(pvks[:7], key_of, flat, xs, check_subgroups=True) == 1
    outside = next(P for label, P, flag in subgroup_cases(name, True)[0] if flag == 0)
    out = flat.copy()
    out[n - 2, 2 * L: 6 * L] = to_arr([outside], name, True)[0]
    assert prover.verify_aggregate_mixed_verdict(pvks[:7], key_of, out, xs, coeffs, check_subgroups=True) == 3
    off = out.copy()
    off[1, 2 * L - 1] ^= np.uint64(1) << np.uint64(20)
    assert prover.verify_aggregate_mixed_verdict(pvks[:7], key_of, off, xs, coeffs, check_subgroups=True) == 2


def test_or_each_names_the_culprits(setup):
    name, prover, keys, pvks, cp = setup
    flat, key_of, xs = batch(keys[:7], [3, 2, 4, 5, 1, 2, 6], "shuffled", seed=6)
    assert prover.verify_proofs_aggregate_mixed_or_each(pvks[:7], key_of, flat, xs).all()
    cases = tamperings(keys[2].proofs, keys[2].vectors[0], cp)
    i, j = positions_of(key_of, 2)[0], positions_of(key_of, 2)[-1]
    flat[i], flat[j] = cases[3][1], cases[6][1]
    got = prover.verify_proofs_aggregate_mixed_or_each(pvks[:7], key_of, flat, xs)
    assert sorted(np.flatnonzero(~got)) == sorted([i, j])


def test_errors_and_the_first_device_rule(setup):
    name, prover, keys, pvks, cp = setup
    flat, key_of, xs = batch(keys[:3], [2, 1, 2])
    n = len(key_of)

    def status(*args, **kw):
        with pytest.raises(g.G16Error) as err:
            prover.verify_aggregate_mixed_verdict(*args, **kw)
        return err.value

    over = key_of.copy()
    over[n - 1] = 3
    assert status(pvks[:3], over, flat, xs).status == 3                     # key_of out of range
    assert status([], key_of, flat, xs).status == 3                         # proofs but no keys
    assert status([pvks[0], None, pvks[2]], key_of, flat, xs).status == 3   # a NULL key
    assert status(pvks[:3], key_of, flat, xs, [1, 2, 0, 4, 5]).status == 3  # a zero coefficient
    x = xs[0]
    assert isinstance(status(pvks[:3], key_of, flat, [np.concatenate([x, x[:1]])] + xs[1:]), g.MalformedVerifyingKey)
    assert isinstance(status(pvks[:3], key_of, flat, [x[:0]] + xs[1:], [1] * n), g.MalformedVerifyingKey)
    other = NAMES[1 - NAMES.index(name)]
    with g.Groth16(other, device=0) as foreign:
        alien = foreign.prepare_verifying_key(mixed_keys(other, 1)[0].vk)
        try:
            assert status([pvks[0], alien, pvks[2]], key_of, flat, xs).status == 3   # a key of another curve
        finally:
            alien.close()
    with g.Groth16(name, device=[0, 0]) as multi:
        theirs = [multi.prepare_verifying_key(c.vk) for c in keys[:3]]
        try:
            assert status([pvks[0], theirs[1], pvks[2]], key_of, flat, xs).status == 3   # a key loaded on another context
            # a multi-device context runs the whole call on its first device
            assert multi.verify_aggregate_mixed_verdict(theirs, key_of, flat, xs, coeffs_for(n, 1)) == 1
            wrong = key_of.copy()
            wrong[0] = 1
            assert multi.verify_aggregate_mixed_verdict(theirs, wrong, flat, xs, coeffs_for(n, 1)) == 0
        finally:
            for p in theirs:
                p.close()
