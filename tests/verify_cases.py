"""Shared fixtures of the verifier tests: keys and proofs from the CPU oracle and from pymodel, and the tamperings of a proof."""
import functools

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


# ---- pairing inputs outside the prime-order subgroups (the plain verifier accepts any on-curve B) ---------------------------------
def nonsubgroup_pairs(curve: str):
    """[(label, [(P, Q)])]: pairs whose G2 point is S + T_l, S in the subgroup and T_l a torsion point of prime order l from
    subgroup_cases.cases -- the two smallest l of G2's cofactor (BN254's has one prime below 2^20) -- and on BLS12-381 the same for
    G1.  [k](S + T_l) is never the identity, so the big-int model's affine chain never divides by zero there."""
    import subgroup_cases as sc
    cp = pm.CURVES[curve]
    G1, G2 = sc.model_groups(cp)
    S1, S2 = G1.mul(cp.g1, 0xC0FFEE), G2.mul(cp.g2, 0xFACADE)
    out = []
    for l, T in list(sc.cases(curve, 1)[1].items())[:2]:
        Q = G2.add(S2, T)
        assert G2.on_curve(Q) and G2.mul(Q, cp.r) is not None
        out.append(("G2 = S + T_%d" % l, [(S1, Q)]))
    for l, T in list(sc.cases(curve, 0)[1].items())[:2]:
        P = G1.add(S1, T)
        assert G1.on_curve(P) and G1.mul(P, cp.r) is not None
        out.append(("G1 = S + T_%d" % l, [(P, S2)]))
    return out


@functools.lru_cache(maxsize=None)
def nonsubgroup_pairs_with_model(curve: str):
    """[(label, pairs, the model's GT limbs)], computed once per process (the big-int pairing takes about a second)"""
    import pairing_model as pmod
    return [(label, pairs, pmod.to_ark_limbs(curve, pmod.pairing_product(curve, pairs))) for label, pairs in nonsubgroup_pairs(curve)]


def torsion_pair(curve: str):
    """(l, P, T_l, hits): Q = T_l of the smallest prime order l >= 11 in G2's cofactor, and whether the Miller loop's chain of
    multiples of Q (the prefixes of |x| on BLS12-381, of the NAF of 6 x + 2 on BN254) reaches a multiple of l, where the projective T
    passes through z = 0 and an affine model has no value"""
    import pairing_model as pmod
    import subgroup_cases as sc
    cp = pm.CURVES[curve]
    tors = sc.cases(curve, 1)[1]
    l = min(k for k in tors if k >= 11)
    x = pmod.LOOP[curve]["x"]
    n = abs(x) if curve == "bls12_381" else 6 * x + 2
    digits = []          # the non-adjacent form, least significant digit first (plain bits for BLS12-381's |x|)
    while n:
        d = (2 - n % 4 if n & 1 else 0) if curve == "bn254" else n & 1
        digits.append(d)
        n = (n - d) // 2
    v, hits = 0, False
    for d in reversed(digits):
        v = 2 * v + d
        hits = hits or v % l == 0
    return l, pm.groups(cp)[0].mul(cp.g1, 0xBADC0DE), tors[l], hits


def identity_ic_case(curve: str, n: int = 3):
    """A key and proofs from known scalars, made with pymodel's groups, whose prepared input IC is the identity:
    gamma_abc_g1 = [-k G, G] and the public input k.  Proof i is A = a G1, B = b G2, C = c G1 with c = (a b - alpha beta) / delta
    mod r, which satisfies e(A, B) = e(alpha, beta) e(IC, gamma) e(C, delta) exactly when IC contributes nothing.  With the input
    k + 1 the prepared input is G and the equation fails.  Returns (vk, [flat proofs], x_good, x_bad, cp)."""
    cp = pm.CURVES[curve]
    G1, G2 = pm.groups(cp)
    r = cp.r
    rng = pm.SplitMix64(0x1C0 + len(curve))
    alpha, beta, gamma, delta, k = (rng.field(r - 1) + 1 for _ in range(5))
    gabc = [G1.neg(G1.mul(cp.g1, k)), cp.g1]
    assert G1.add(gabc[0], G1.mul(gabc[1], k)) is None and G1.add(gabc[0], G1.mul(gabc[1], (k + 1) % r)) == cp.g1
    vk = g.VerifyingKey(curve, g1_to_arr([G1.mul(cp.g1, alpha)], cp)[0], g2_to_arr([G2.mul(cp.g2, beta)], cp)[0],
                        g2_to_arr([G2.mul(cp.g2, gamma)], cp)[0], g2_to_arr([G2.mul(cp.g2, delta)], cp)[0], g1_to_arr(gabc, cp))
    proofs = []
    for _ in range(n):
        a, b = rng.field(r - 1) + 1, rng.field(r - 1) + 1
        c = (a * b - alpha * beta) * pow(delta, -1, r) % r
        assert (a * b - alpha * beta - c * delta) % r == 0 and (a * b - alpha * beta - gamma - c * delta) % r != 0
        proofs.append(np.concatenate([g1_to_arr([G1.mul(cp.g1, a)], cp)[0], g2_to_arr([G2.mul(cp.g2, b)], cp)[0],
                                      g1_to_arr([G1.mul(cp.g1, c)], cp)[0]]))
    x_good = ints_to_mont([k], r, 4).reshape(-1, 4)
    x_bad = ints_to_mont([(k + 1) % r], r, 4).reshape(-1, 4)
    return vk, proofs, x_good, x_bad, cp
