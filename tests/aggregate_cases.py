"""Shared by the aggregate-verifier tests: batches of honest, tampered and cancelling proofs, and the verdict rule of the batch."""
import random

import pymodel as pm
from helpers import arr_to_g1, g1_to_arr

import groth16_amd as g


def as_proof(flat, cp):
    L = cp.fq_limbs64
    return g.Proof(flat[: 2 * L].copy(), flat[2 * L: 6 * L].copy(), flat[6 * L:].copy())


def honest_base(name, vk, proofs, cp, extra=3, seed=17):
    """the two honest proofs of a case and `extra` rerandomisations of the first"""
    rng = random.Random(seed)
    base = [p.copy() for p in proofs]
    for _ in range(extra):
        base.append(g.rerandomize_proof(name, vk, as_proof(proofs[0], cp), rng).flat())
    return base


def expected_verdict(verdicts):
    """1 if every per-proof verdict is 1, else 2 if any is 2, else 0"""
    v = list(verdicts)
    return 1 if all(x == 1 for x in v) else 2 if any(x == 2 for x in v) else 0


def coeffs_for(n, seed):
    """n non-zero 128-bit coefficients from a seeded generator (tests only: the library's own draw uses the operating system)"""
    rng = random.Random(seed)
    return [rng.getrandbits(128) | 1 for _ in range(n)]


def cancelling_pair(p, q, cp):
    """p' = (A_p, B_p, C_p + D), q' = (A_q, B_q, C_q - D) with D = A_p: each fails verify_proof, and the plain product of the two
    equations holds because the D terms cancel"""
    L = cp.fq_limbs64
    G1, _ = pm.groups(cp)
    d = arr_to_g1(p[: 2 * L], cp)[0]
    cp_, cq_ = arr_to_g1(p[6 * L:], cp)[0], arr_to_g1(q[6 * L:], cp)[0]
    p2, q2 = p.copy(), q.copy()
    p2[6 * L:] = g1_to_arr([G1.add(cp_, d)], cp)[0]
    q2[6 * L:] = g1_to_arr([G1.add(cq_, G1.neg(d))], cp)[0]
    return p2, q2
