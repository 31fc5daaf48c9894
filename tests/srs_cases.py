"""Setup from an SRS: a literal big-int model and the cases the CPU and GPU tiers share (TEST INFRASTRUCTURE).

The model works on pymodel's group arithmetic alone and follows the derivation step by step:
  model_srs            tau^i G1, tau^i G2, alpha tau^i G1, beta tau^i G1, beta G2 from known secrets
  model_group_dft      out[i] = sum_k root^(ik) P[k] as a plain sum over points (any size; used up to 32 points)
  model_key_from_srs   1. u = the inverse n-point transform of the SRS powers (four times), 2. the column sums of A, B, C over u,
                       3. h_query (Libsnark: tau_g1[i + n] - tau_g1[i]; Circom: the odd outputs of the inverse 2n-point transform)
and, independent of all that, the same key IN THE EXPONENT from the toxic waste with gamma = delta = 1:
  trapdoor_key         pymodel's instance_map_with_evaluation / circom_model's h_query_scalars, then scalar * generator."""
import numpy as np

import circom_model as cm
import pymodel as pm
from helpers import circuit_from_pymodel, g1_to_arr, g2_to_arr, ints_to_mont

CURVES = [pm.BLS12_381, pm.BN254]
LIBSNARK, CIRCOM = 0, 1
KEY_FIELDS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2", "gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query",
              "h_query", "l_query")
G2_FIELDS = ("beta_g2", "delta_g2", "gamma_g2", "b_g2_query")


def fr(cp, v) -> np.ndarray:
    return ints_to_mont([v], cp.r, 4)[0].copy()


def secrets(cp, seed: int = 41):
    """tau, alpha, beta, delta and a non-standard pair of generators"""
    rng = pm.SplitMix64(seed)
    G1, G2 = pm.groups(cp)
    tau, alpha, beta, delta = (rng.field(cp.r - 1) + 1 for _ in range(4))
    return dict(tau=tau, alpha=alpha, beta=beta, delta=delta, g1=G1.mul(cp.g1, rng.field(cp.r - 1) + 1), g2=G2.mul(cp.g2, rng.field(cp.r - 1) + 1))


def domain_size(cs) -> int:
    n = 1
    while n < cs.num_constraints + cs.num_inputs:
        n <<= 1
    return n


def model_srs(cp, n: int, sec, extra: int = 0):
    """the SRS a domain of n points needs (+ `extra` points on every array)"""
    G1, G2 = pm.groups(cp)
    p = cp.r
    pw = [pow(sec["tau"], i, p) for i in range(2 * n - 1 + extra)]
    m = n + extra
    return dict(tau_g1=[G1.mul(sec["g1"], s) for s in pw], tau_g2=[G2.mul(sec["g2"], s) for s in pw[:m]],
                alpha_tau_g1=[G1.mul(sec["g1"], sec["alpha"] * s % p) for s in pw[:m]],
                beta_tau_g1=[G1.mul(sec["g1"], sec["beta"] * s % p) for s in pw[:m]], beta_g2=[G2.mul(sec["g2"], sec["beta"])])


def srs_to_arrays(g, cp, srs):
    """a model SRS as groth16_amd.SRS"""
    return g.SRS(cp.name, g1_to_arr(srs["tau_g1"], cp), g2_to_arr(srs["tau_g2"], cp), g1_to_arr(srs["alpha_tau_g1"], cp),
                 g1_to_arr(srs["beta_tau_g1"], cp), g2_to_arr(srs["beta_g2"], cp))


def model_group_dft(G, pts, root: int, p: int, scale: int = 1):
    m = len(pts)
    return [G.msm(pts, [scale * pow(root, i * k, p) % p for k in range(m)]) for i in range(m)]


def _col_sum(G, rows, pts, nv, p, init=None):
    acc = list(init) if init is not None else [None] * nv
    for i, row in enumerate(rows):
        for cf, idx in row:
            if cf % p and pts[i] is not None:
                acc[idx] = G.add(acc[idx], G.mul(pts[i], cf % p))
    return acc


def model_key_from_srs(cp, cs, srs, qap: int):
    """steps 1-3, literally, over points"""
    G1, G2 = pm.groups(cp)
    p = cp.r
    n = domain_size(cs)
    assert n <= 16, "the model sums n^2 scalar multiplications"
    w, rho = cm.roots(cp, n)
    w_inv, n_inv = pow(w, p - 2, p), pow(n, p - 2, p)
    u = model_group_dft(G1, srs["tau_g1"][:n], w_inv, p, n_inv)
    au = model_group_dft(G1, srs["alpha_tau_g1"][:n], w_inv, p, n_inv)
    bu = model_group_dft(G1, srs["beta_tau_g1"][:n], w_inv, p, n_inv)
    u2 = model_group_dft(G2, srs["tau_g2"][:n], w_inv, p, n_inv)
    ni, nc = cs.num_inputs, cs.num_constraints
    nv = ni + cs.num_witness
    inst = lambda v: [v[nc + j] if j < ni else None for j in range(nv)]  # noqa: E731
    a = _col_sum(G1, cs.a, u, nv, p, inst(u))
    b1 = _col_sum(G1, cs.b, u, nv, p)
    b2 = _col_sum(G2, cs.b, u2, nv, p)
    m = _col_sum(G1, cs.c, u, nv, p, _col_sum(G1, cs.b, au, nv, p, _col_sum(G1, cs.a, bu, nv, p, inst(bu))))
    t1 = srs["tau_g1"]
    if qap == LIBSNARK:
        h = [G1.add(t1[i + n], G1.neg(t1[i])) for i in range(n - 1)]
    else:
        h = model_group_dft(G1, t1[:2 * n - 1] + [None], pow(rho, p - 2, p), p, pow(2 * n, p - 2, p))[1::2]
    return dict(alpha_g1=[srs["alpha_tau_g1"][0]], beta_g1=[srs["beta_tau_g1"][0]], delta_g1=[t1[0]], beta_g2=[srs["beta_g2"][0]],
                delta_g2=[srs["tau_g2"][0]], gamma_g2=[srs["tau_g2"][0]], gamma_abc_g1=m[:ni], a_query=a, b_g1_query=b1, b_g2_query=b2,
                h_query=h, l_query=m[ni:])


def trapdoor_key(cp, cs, sec, qap: int, delta: int = 1):
    """the same key in the exponent: gamma = 1, t = tau"""
    G1, G2 = pm.groups(cp)
    p = cp.r
    t, alpha, beta = sec["tau"], sec["alpha"], sec["beta"]
    a, b, c, zt, m, n = pm.instance_map_with_evaluation(cp, cs, t)
    ni = cs.num_inputs
    di = pow(delta, p - 2, p)
    mm = [(beta * a[i] + alpha * b[i] + c[i]) % p for i in range(m + 1)]
    if qap == LIBSNARK:
        hs = [zt * di % p * pow(t, i, p) % p for i in range(n - 1)]
    else:
        hs = cm.h_query_scalars(cp, n, t, di)
    bm = lambda G, gen, sc: [G.mul(gen, s % p) if s % p else None for s in sc]  # noqa: E731
    g1, g2 = sec["g1"], sec["g2"]
    return dict(alpha_g1=bm(G1, g1, [alpha]), beta_g1=bm(G1, g1, [beta]), delta_g1=bm(G1, g1, [delta]), beta_g2=bm(G2, g2, [beta]),
                delta_g2=bm(G2, g2, [delta]), gamma_g2=bm(G2, g2, [1]), gamma_abc_g1=bm(G1, g1, mm[:ni]), a_query=bm(G1, g1, a),
                b_g1_query=bm(G1, g1, b), b_g2_query=bm(G2, g2, b), h_query=bm(G1, g1, hs), l_query=bm(G1, g1, [x * di for x in mm[ni:]]))


def key_to_arrays(cp, key) -> dict:
    return {f: (g2_to_arr if f in G2_FIELDS else g1_to_arr)(key[f], cp) for f in KEY_FIELDS}


def assert_keys_equal(got, want, label=""):
    """field by field, byte for byte; `got` a groth16_amd.ProvingKey, `want` another one or a dict of arrays"""
    for f in KEY_FIELDS:
        w = want[f] if isinstance(want, dict) else getattr(want, f)
        x = getattr(got, f)
        assert x.shape == w.shape or x.size == w.size, (label, f, x.shape, w.shape)
        assert (x.reshape(-1) == np.asarray(w).reshape(-1)).all(), (label, f)


def mats_of(g, ck):
    return g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints, *[(m.row_ptr, m.col, m.val) for m in ck.abc])


def host_circuits(cp):
    """(name, R1CS, z): syn k = 2 and 4, and a MiMC circuit whose domain is padded (10 + 2 rows in 16)"""
    yield ("syn2",) + pm.syn_circuit(cp, 2, 3)
    yield ("syn4",) + pm.syn_circuit(cp, 4, 5)
    cs, z = pm.mimc_circuit(cp, 5, 2)
    assert domain_size(cs) != cs.num_constraints + cs.num_inputs
    yield "mimc5", cs, z


def flat(cp, cs, z):
    return circuit_from_pymodel(cp, cs, z)
