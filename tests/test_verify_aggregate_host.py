"""CPU tier: the randomised batch verifier on the host (g16_host_verify_aggregate runs the per-proof function and the tail that
g16_verify_aggregate uses) against per-proof verdicts, the cancelling-pair attack and the big-int pairing model."""
import random

import numpy as np
import pytest

import pairing_model as pmod
import pymodel as pm
from aggregate_cases import cancelling_pair, coeffs_for, expected_verdict, honest_base
from helpers import arr_to_g1, arr_to_g2, mont_to_ints
from verify_cases import oracle_case, pymodel_case, tamperings

import groth16_amd as g
from groth16_amd.verifier import host_aggregate_gt, host_aggregate_verdict, host_verdict

NAMES = ["bls12_381", "bn254"]
MAKERS = pytest.mark.parametrize("make", [oracle_case, pymodel_case], ids=["oracle_syn", "pymodel_mimc"])


@MAKERS
@pytest.mark.parametrize("name", NAMES)
def test_honest_batch_is_accepted(name, make):
    vk, proofs, x, cp = make(name)
    base = honest_base(name, vk, proofs, cp, extra=4)
    xs = [x] * len(base)
    assert host_aggregate_verdict(name, vk, base, xs, coeffs_for(len(base), 1)) == 1
    assert host_aggregate_verdict(name, vk, np.stack(base), xs, np.array([[1, 0]] * len(base), dtype=np.uint64)) == 1
    assert host_aggregate_verdict(name, vk, base, xs, None) == 1
    assert g.verify_proofs_aggregate_host(name, vk, base, xs)


@MAKERS
@pytest.mark.parametrize("name", NAMES)
def test_one_tampered_proof_among_honest_ones(name, make):
    """rule: 1 if every host_verdict of the batch is 1, else 2 if any is 2, else 0.  With one invalid proof the residual is a
    non-trivial GT element raised to r_i, 0 < r_i < 2^128 < r: the rejection is exact for any non-zero coefficient."""
    vk, proofs, x, cp = make(name)
    base = honest_base(name, vk, proofs, cp, extra=2)
    rng = random.Random(5)
    for k, (label, proof, xi, want) in enumerate(tamperings(proofs, x, cp)):
        batch, xs = [b.copy() for b in base], [x] * len(base)
        pos = rng.randrange(len(batch))
        batch[pos], xs[pos] = proof, xi
        each = [host_verdict(name, vk, p, xv) for p, xv in zip(batch, xs)]
        assert each[pos] == want, label
        rule = expected_verdict(each)
        assert host_aggregate_verdict(name, vk, batch, xs, coeffs_for(len(batch), 100 + k)) == rule, label
        if k % 3 == 0:
            assert host_aggregate_verdict(name, vk, batch, xs, None) == rule, label


@pytest.mark.parametrize("name", NAMES)
def test_cancelling_pair_needs_distinct_coefficients(name):
    """With all coefficients 1 the aggregate is the plain product of the equations and ACCEPTS two invalid proofs whose errors
    cancel -- asserted to document the attack.  Distinct coefficients leave e((r_1 - r_2) D, delta) != 1: exact rejection."""
    vk, proofs, x, cp = oracle_case(name)
    p2, q2 = cancelling_pair(proofs[0], proofs[1], cp)
    assert host_verdict(name, vk, p2, x) == 0 and host_verdict(name, vk, q2, x) == 0
    honest = honest_base(name, vk, proofs, cp, extra=1)[2]
    for batch in ([p2, q2], [p2, honest, q2]):
        xs = [x] * len(batch)
        assert host_aggregate_verdict(name, vk, batch, xs, [1] * len(batch)) == 1
        assert host_aggregate_verdict(name, vk, batch, xs, list(range(1, len(batch) + 1))) == 0
        assert host_aggregate_verdict(name, vk, batch, xs, None) == 0


@pytest.mark.parametrize("name", NAMES)
def test_both_sides_equal_the_pairing_model(name):
    """the GT values the equation compares: the model's pairing product over the 3 + 2 pairs, and e(alpha, beta)^s"""
    vk, proofs, x, cp = oracle_case(name)
    L = cp.fq_limbs64
    G1, G2 = pm.groups(cp)
    F = pm.Fq12(cp)
    batch = honest_base(name, vk, proofs, cp, extra=1)
    coeffs = [3, (1 << 127) + 12345, 0xFEDCBA9876543210_0123456789ABCDEF]
    xs = [x, x, x]
    lhs, rhs = host_aggregate_gt(name, vk, batch, xs, coeffs)
    gabc = arr_to_g1(vk.gamma_abc_g1, cp)
    xi = mont_to_ints(x.reshape(-1, 4), cp.r)
    s = sum(coeffs) % cp.r
    pairs, s_ic, s_c = [], G1.mul(gabc[0], s), None
    for r, flat in zip(coeffs, batch):
        pairs.append((G1.mul(arr_to_g1(flat[: 2 * L], cp)[0], r), arr_to_g2(flat[2 * L: 6 * L], cp)[0]))
        s_c = G1.add(s_c, G1.mul(arr_to_g1(flat[6 * L:], cp)[0], r))
    for j, v in enumerate(xi):
        s_ic = G1.add(s_ic, G1.mul(gabc[j + 1], sum(coeffs) * v % cp.r))
    pairs.append((s_ic, G2.neg(arr_to_g2(vk.gamma_g2, cp)[0])))
    pairs.append((s_c, G2.neg(arr_to_g2(vk.delta_g2, cp)[0])))
    assert (lhs == pmod.to_ark_limbs(name, pmod.pairing_product(name, pairs))).all()
    ab = pmod.pairing(name, arr_to_g1(vk.alpha_g1, cp)[0], arr_to_g2(vk.beta_g2, cp)[0])
    assert (rhs == pmod.to_ark_limbs(name, F.pow(ab, s))).all()
    assert (lhs == rhs).all()


@pytest.mark.parametrize("name", NAMES)
def test_edges(name):
    vk, proofs, x, cp = oracle_case(name)
    L = cp.fq_limbs64
    assert host_aggregate_verdict(name, vk, [], [], None) == 1
    assert host_aggregate_verdict(name, vk, np.zeros((0, 8 * L), np.uint64), [], []) == 1
    for label, proof, xi, want in tamperings(proofs, x, cp):   # n = 1 equals verify_proof
        assert host_aggregate_verdict(name, vk, [proof], [xi], [0x1234567]) == host_verdict(name, vk, proof, xi) == want, label
    with pytest.raises(g.G16Error) as err:   # a zero coefficient would drop its proof from the check
        host_aggregate_verdict(name, vk, proofs, [x, x], [5, 0])
    assert err.value.status == 3 and not isinstance(err.value, g.SynthesisError)
    with pytest.raises(g.MalformedVerifyingKey):
        host_aggregate_verdict(name, vk, proofs, [np.concatenate([x, x[:1]])] * 2, [1, 2])
    with pytest.raises(g.MalformedVerifyingKey):
        host_aggregate_verdict(name, vk, proofs, [x[:0], x[:0]], [1, 2])
    with pytest.raises(ValueError):
        host_aggregate_verdict(name, vk, proofs, [x, x], [1, 2, 3])
    with pytest.raises(ValueError):
        host_aggregate_verdict(name, vk, proofs, [x, x], [1, 1 << 128])
    a0, c0 = proofs[0].copy(), proofs[0].copy()
    a0[: 2 * L] = 0
    c0[6 * L:] = 0
    for bad in (a0, c0):
        assert host_verdict(name, vk, bad, x) == 0
        assert host_aggregate_verdict(name, vk, [proofs[1], bad], [x, x], [7, 9]) == 0
        assert host_aggregate_verdict(name, vk, [bad], [x], None) == 0


@pytest.mark.parametrize("name", NAMES)
def test_no_public_inputs(name):
    """a key with gamma_abc_g1 = [IC] (l = 0): S_IC = s IC"""
    vk, proofs, x, cp = oracle_case(name)
    G1, _ = pm.groups(cp)
    gabc = arr_to_g1(vk.gamma_abc_g1, cp)
    ic = gabc[0]
    for v, base in zip(mont_to_ints(x.reshape(-1, 4), cp.r), gabc[1:]):
        ic = G1.add(ic, G1.mul(base, v))
    from helpers import g1_to_arr
    vk0 = g.VerifyingKey(name, vk.alpha_g1, vk.beta_g2, vk.gamma_g2, vk.delta_g2, g1_to_arr([ic], cp))
    assert host_aggregate_verdict(name, vk0, proofs, [[], []], [11, 13]) == 1
    assert host_aggregate_verdict(name, vk0, proofs, [[], []], None) == 1
    bad = proofs[0].copy()
    bad[6 * cp.fq_limbs64:] = proofs[1][6 * cp.fq_limbs64:]
    assert host_aggregate_verdict(name, vk0, [proofs[1], bad], [[], []], [11, 13]) == 0
    with pytest.raises(g.MalformedVerifyingKey):
        host_aggregate_verdict(name, vk0, proofs, [x, x], [1, 2])
