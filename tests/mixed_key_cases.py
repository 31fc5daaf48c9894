"""Shared by the mixed-key verifier tests (both tiers): verifying keys that really differ, honest proofs under each, and batches
that interleave them.

  oracle_keys   three keys from three set-ups of one circuit (three trapdoors: alpha, beta, gamma, delta all differ).
                verify_cases.oracle_case always sets up with seed 3, so its keys would hide a key mix-up.
  widen         the construction of wide_key in tests/test_gpu_verify_aggregate.py on top of those keys: a key with 0, 1, 3 or 16
                public inputs under which the same proofs verify.
  derive        further keys by big-int group arithmetic, so that 65 keys cost no 65 set-ups.  For scalars a, m, k
                    key'   = (a alpha, beta, m gamma, k delta, a m^-1 gamma_abc)      proof' = (a A, B, a k^-1 C)
                and e(a A, B) = [e(alpha, beta) e(IC, gamma) e(C, delta)]^a = e(a alpha, beta) e(a m^-1 IC, m gamma) e(a k^-1 C, k delta):
                proof' verifies under key' exactly when the proof verifies under the key.  With a = c k and m = c for small c, k
                every scalar that multiplies a point (c k, c, k) is small, which keeps the big-int arithmetic quick; every derived
                key still has its own alpha, gamma, delta, gamma_abc and e(alpha, beta).
The helper checks its own output on the CPU: every proof has host_verdict 1 under its key and 0 under a neighbour's."""
import functools
import random

import numpy as np

import pymodel as pm
from helpers import arr_to_g1, arr_to_g2, g1_to_arr, g2_to_arr, ints_to_mont, mont_to_ints, oracle

import groth16_amd as g
from groth16_amd.verifier import host_verdict

NAMES = ["bls12_381", "bn254"]
SETUP_SEEDS = (3, 11, 23)
WIDTHS = (0, 1, 3, 16)


class KeyCase:
    """a key, honest proofs under it, and public-input vectors each of which goes with every one of the proofs"""

    def __init__(self, vk, proofs, vectors):
        self.vk, self.proofs, self.vectors = vk, proofs, vectors

    @property
    def num_public(self):
        return self.vk.num_public


@functools.lru_cache(maxsize=None)
def oracle_keys(name):
    orc = oracle()
    ck = orc.syn_circuit(name, 4, 9)
    x = np.ascontiguousarray(ck.z[1: ck.num_inputs]).reshape(-1, 4)
    out = []
    for seed in SETUP_SEEDS:
        pk, ex = orc.setup(ck, seed)
        proofs = []
        for i in range(2):
            r, s = orc.rand_fr(name, 5 + 2 * i + seed, 1)[0], orc.rand_fr(name, 6 + 2 * i + seed, 1)[0]
            flat, _ = orc.prove(pk, ck, r, s)
            proofs.append(np.asarray(flat, dtype=np.uint64))
        vk = g.VerifyingKey(name, pk.alpha_g1.reshape(-1), pk.beta_g2.reshape(-1), ex["gamma_g2"].reshape(-1), pk.delta_g2.reshape(-1),
                            np.ascontiguousarray(ex["gamma_abc"]))
        out.append(KeyCase(vk, proofs, [x]))
    return out


def widen(case, cp, n_inputs, n_vectors, seed):
    """gamma_abc'[j] = k_j G for j >= 1 and every input vector x' has sum_j x'_j k_j = c, with gamma_abc'[0] = IC - c G (IC: the
    prepared input of the case's key at its first vector); n_inputs = 0 leaves gamma_abc' = [IC]"""
    G1, _ = pm.groups(cp)
    rng = random.Random(seed)
    vk = case.vk
    gabc = arr_to_g1(vk.gamma_abc_g1, cp)
    ic = gabc[0]
    for v, b in zip(mont_to_ints(case.vectors[0].reshape(-1, 4), cp.r), gabc[1:]):
        ic = G1.add(ic, G1.mul(b, v))
    if n_inputs == 0:
        new, vectors = [ic], [np.zeros((0, 4), dtype=np.uint64)]
    else:
        ks = [rng.randrange(1, cp.r) for _ in range(n_inputs)]
        c = rng.randrange(cp.r)
        new = [G1.add(ic, G1.neg(G1.mul(cp.g1, c)))] + [G1.mul(cp.g1, k) for k in ks]
        vectors = []
        for _ in range(n_vectors):
            v = [rng.randrange(cp.r) for _ in range(n_inputs - 1)]
            rest = (c - sum(a * k for a, k in zip(v, ks))) % cp.r
            v.append(rest * pow(ks[-1], -1, cp.r) % cp.r)
            vectors.append(ints_to_mont(v, cp.r, 4).reshape(-1, 4))
    return KeyCase(g.VerifyingKey(vk.curve, vk.alpha_g1, vk.beta_g2, vk.gamma_g2, vk.delta_g2, g1_to_arr(new, cp)), case.proofs, vectors)


def derive(case, cp, c, k):
    """key' and proof' of the module docstring for a = c k, m = c: (c k alpha, beta, c gamma, k delta, k gamma_abc), (c k A, B, c C)"""
    G1, G2 = pm.groups(cp)
    L = cp.fq_limbs64
    vk = case.vk
    g1 = lambda arr, s: g1_to_arr([G1.mul(p, s) for p in arr_to_g1(arr, cp)], cp)
    g2 = lambda arr, s: g2_to_arr([G2.mul(p, s) for p in arr_to_g2(arr, cp)], cp)
    new = g.VerifyingKey(vk.curve, g1(vk.alpha_g1, c * k).reshape(-1), vk.beta_g2, g2(vk.gamma_g2, c).reshape(-1), g2(vk.delta_g2, k).reshape(-1),
                         g1(vk.gamma_abc_g1, k))
    proofs = []
    for p in case.proofs:
        q = p.copy()
        q[: 2 * L] = g1(p[: 2 * L], c * k).reshape(-1)
        q[6 * L:] = g1(p[6 * L:], c).reshape(-1)
        proofs.append(q)
    return KeyCase(new, proofs, case.vectors)


def self_check(name, keys):
    for i, case in enumerate(keys):
        other = next((keys[j % len(keys)] for j in range(i + 1, i + len(keys)) if keys[j % len(keys)].num_public == case.num_public), None)
        for t, p in enumerate(case.proofs):
            x = case.vectors[t % len(case.vectors)]
            assert host_verdict(name, case.vk, p, x) == 1, (name, i, t)
            if other is not None:
                assert host_verdict(name, other.vk, p, x) == 0, (name, i, t)


@functools.lru_cache(maxsize=None)
def mixed_keys(name, count):
    """`count` different keys: the three oracle keys, then derived keys with 0, 1, 3 and 16 public inputs, then derived copies of
    all of those in turn"""
    cp = pm.CURVES[name]
    rng = random.Random(1000 + NAMES.index(name))
    scalars = rng.sample(range(2, 1 << 20), 2 * max(count, 8))
    keys = list(oracle_keys(name))
    for i, w in enumerate(WIDTHS):
        if len(keys) >= count:
            break
        keys.append(derive(widen(keys[i % 3], cp, w, 3, seed=40 + i), cp, scalars[2 * len(keys)], scalars[2 * len(keys) + 1]))
    while len(keys) < count:
        keys.append(derive(keys[len(keys) % 7], cp, scalars[2 * len(keys)], scalars[2 * len(keys) + 1]))
    keys = keys[:count]
    self_check(name, keys)
    return keys


def batch(keys, sizes, order="grouped", seed=0):
    """(flat proofs (n, words), key_of (n,) uint32, input vectors) of sizes[k] honest proofs under keys[k], in one of three orders:
    grouped by key, round-robin over the keys, shuffled"""
    items = []
    for k, (case, m) in enumerate(zip(keys, sizes)):
        for t in range(m):
            items.append((t, k, case.proofs[t % len(case.proofs)], case.vectors[(t // 2) % len(case.vectors)]))
    if order == "round_robin":
        items.sort(key=lambda it: (it[0], it[1]))
    elif order == "shuffled":
        random.Random(seed).shuffle(items)
    else:
        assert order == "grouped", order
    flat = np.stack([it[2] for it in items])
    return flat, np.array([it[1] for it in items], dtype=np.uint32), [it[3] for it in items]


def positions_of(key_of, k):
    return [int(i) for i in np.flatnonzero(np.asarray(key_of) == k)]
