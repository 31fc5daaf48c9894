"""Shared fixtures of the verifier tests: keys and proofs from the CPU oracle and from pymodel, and the tamperings of a proof."""
import numpy as np

import pymodel as pm
from helpers import g1_to_arr, g2_to_arr, ints_to_mont, mont_to_ints, oracle

import groth16_amd as g


def oracle_case(curve: str, k: int = 4, seed: int = 9):
    """(VerifyingKey, [flat proof, flat proof of other r/s], public inputs (Montgomery Fr rows), pymodel vk, cp)"""
    orc = oracle()
    cp = pm.CURVES[curve]
    ck = orc.syn_circuit(curve, k, seed)
    pk, ex = orc.setup(ck, 3)
    proofs = []
    for i in range(2):
        r, s = orc.rand_fr(curve, 5 + 2 * i, 1)[0], orc.rand_fr(curve, 6 + 2 * i, 1)[0]
        flat, _ = orc.prove(pk, ck, r, s)
        proofs.append(np.asarray(flat, dtype=np.uint64))
    vk = g.VerifyingKey(curve, pk.alpha_g1.reshape(-1), pk.beta_g2.reshape(-1), ex["gamma_g2"].reshape(-1), pk.delta_g2.reshape(-1),
                        np.ascontiguousarray(ex["gamma_abc"]))
    x = np.ascontiguousarray(ck.z[1: ck.num_inputs]).reshape(-1, 4)
    return vk, proofs, x, cp


def pymodel_case(curve: str, rounds: int = 4, seed: int = 3):
    """the same from pymodel's own setup and prover on a MiMC circuit"""
    cp = pm.CURVES[curve]
    cs, z = pm.mimc_circuit(cp, rounds, seed)
    pk, _ = pm.generate_parameters(cp, cs, 5)
    proofs = []
    for i in range(2):
        r, s = pm.SplitMix64(1 + 2 * i).field(cp.r), pm.SplitMix64(2 + 2 * i).field(cp.r)
        pr = pm.create_proof_with_reduction_and_matrices(cp, pk, r, s, cs, z)
        proofs.append(np.concatenate([g1_to_arr([pr.a], cp)[0], g2_to_arr([pr.b], cp)[0], g1_to_arr([pr.c], cp)[0]]))
    vk = g.VerifyingKey(curve, g1_to_arr([pk.alpha_g1], cp)[0], g2_to_arr([pk.beta_g2], cp)[0], g2_to_arr([pk.gamma_g2], cp)[0],
                        g2_to_arr([pk.delta_g2], cp)[0], g1_to_arr(pk.gamma_abc_g1, cp))
    x = ints_to_mont(z[1: cs.num_inputs], cp.r, 4).reshape(-1, 4)
    return vk, proofs, x, cp


def pm_vk(vk: "g.VerifyingKey", cp):
    from helpers import arr_to_g1, arr_to_g2
    return pm.ProvingKey(arr_to_g1(vk.alpha_g1, cp)[0], None, arr_to_g2(vk.beta_g2, cp)[0], None, arr_to_g2(vk.delta_g2, cp)[0],
                         arr_to_g2(vk.gamma_g2, cp)[0], arr_to_g1(vk.gamma_abc_g1, cp), [], [], [], [], [])


def pm_proof(flat, cp):
    from helpers import arr_to_g1, arr_to_g2
    L = cp.fq_limbs64
    return pm.Proof(arr_to_g1(flat[: 2 * L], cp)[0], arr_to_g2(flat[2 * L: 6 * L], cp)[0], arr_to_g1(flat[6 * L:], cp)[0])


def wrong_input(x, cp):
    v = mont_to_ints(x.reshape(-1, 4), cp.r)
    v[0] = (v[0] + 1) % cp.r
    return ints_to_mont(v, cp.r, 4).reshape(-1, 4)


def neg_g1(p, cp):
    L = cp.fq_limbs64
    xy = mont_to_ints(p.reshape(2, L), cp.q)
    if not any(xy):
        return p.copy()
    return ints_to_mont([xy[0], (-xy[1]) % cp.q], cp.q, L).reshape(-1)


def tamperings(proofs, x, cp):
    """[(name, flat proof, public inputs, expected verdict)] -- src/test.rs:71 and the substitutions of the issue"""
    L = cp.fq_limbs64
    p, q = proofs
    c_is_a = p.copy()
    c_is_a[6 * L:] = p[: 2 * L]
    b_other = p.copy()
    b_other[2 * L: 6 * L] = q[2 * L: 6 * L]
    a_neg = p.copy()
    a_neg[: 2 * L] = neg_g1(p[: 2 * L], cp)
    off = p.copy()
    off[2 * L - 1] ^= np.uint64(1) << np.uint64(20)   # A.y changed: not on the curve
    off_b = p.copy()
    off_b[2 * L] ^= np.uint64(1)                       # B.x changed
    return [("honest", p, x, 1), ("honest2", q, x, 1), ("wrong_input", p, wrong_input(x, cp), 0), ("c_is_a", c_is_a, x, 0),
            ("b_other", b_other, x, 0), ("a_neg", a_neg, x, 0), ("off_curve_a", off, x, 2), ("off_curve_b", off_b, x, 2)]
