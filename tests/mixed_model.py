"""The mixed-key aggregate equation written literally over the big-int pairing model (pairing_model.py):

    FE( prod_i ML(r_i A_i, B_i) * prod_k [ ML(S_IC_k, -gamma_k) * ML(S_C_k, -delta_k) ] )  ==  prod_k e(alpha_k, beta_k)^(s_k)
    s_k = sum_{i in k} r_i      t_kj = sum_{i in k} r_i x_ij
    S_IC_k = s_k gamma_abc_k[0] + sum_j t_kj gamma_abc_k[j+1]      S_C_k = sum_{i in k} r_i C_i
"""
import pairing_model as pmod
import pymodel as pm
from helpers import arr_to_g1, arr_to_g2, mont_to_ints


def mixed_gt(name, vks, key_of, proofs, xs, coeffs):
    """(lhs, rhs) as pymodel Fq12 values; vks: groth16_amd.VerifyingKey, proofs: flat arrays, xs: Montgomery Fr rows per proof"""
    cp = pm.CURVES[name]
    L = cp.fq_limbs64
    G1, G2 = pm.groups(cp)
    F = pm.Fq12(cp)
    pairs = [(G1.mul(arr_to_g1(p[: 2 * L], cp)[0], r), arr_to_g2(p[2 * L: 6 * L], cp)[0]) for p, r in zip(proofs, coeffs)]
    rhs = F.one
    for k, vk in enumerate(vks):
        mine = [i for i in range(len(proofs)) if key_of[i] == k]
        if not mine:
            continue
        gabc = arr_to_g1(vk.gamma_abc_g1, cp)
        s_k = sum(coeffs[i] for i in mine) % cp.r
        s_ic = G1.mul(gabc[0], s_k)
        for j in range(len(gabc) - 1):
            t_kj = sum(coeffs[i] * mont_to_ints(xs[i].reshape(-1, 4), cp.r)[j] for i in mine) % cp.r
            s_ic = G1.add(s_ic, G1.mul(gabc[j + 1], t_kj))
        s_c = None
        for i in mine:
            s_c = G1.add(s_c, G1.mul(arr_to_g1(proofs[i][6 * L:], cp)[0], coeffs[i]))
        pairs.append((s_ic, G2.neg(arr_to_g2(vk.gamma_g2, cp)[0])))
        pairs.append((s_c, G2.neg(arr_to_g2(vk.delta_g2, cp)[0])))
        ab = pmod.pairing(name, arr_to_g1(vk.alpha_g1, cp)[0], arr_to_g2(vk.beta_g2, cp)[0])
        rhs = F.mul(rhs, F.pow(ab, s_k))
    return pmod.pairing_product(name, pairs), rhs
