"""Shared by the decompression tests (both tiers): per curve and per group a list of compressed encodings with the status and the
affine point the big-int model gives them.  Encodings come from pymodel.compress_* (valid ones) and from raw integers with chosen
flag bits (invalid ones); square roots from subgroup_cases.sqrt_fq / sqrt_fq2.  cases() also holds every expected status against
g16_deserialize_points(compressed=1, validate=0), one point at a time, and every expected point against the model."""
import functools

import numpy as np

import pymodel as pm
from subgroup_cases import NAMES, model_groups, random_curve_point, sqrt_fq, sqrt_fq2, to_arr

import groth16_amd as g
from groth16_amd.serialize import deserialize_points, serialize_points


def fq_bytes(name):
    return 48 if name == "bls12_381" else 32


def enc_size(name, g2):
    return fq_bytes(name) * (2 if g2 else 1)


def compress(name, g2, P):
    fn = {("bls12_381", 0): pm.compress_g1_bls, ("bls12_381", 1): pm.compress_g2_bls, ("bn254", 0): pm.compress_g1_bn,
          ("bn254", 1): pm.compress_g2_bn}[(name, int(g2))]
    return fn(P)


def raw(name, g2, x, inf=False, sign=False, compressed_bit=True):
    """an encoding from raw integers (not reduced, so x >= p can be written) and explicit flag bits"""
    n = fq_bytes(name)
    if name == "bls12_381":
        b = bytearray((x[1].to_bytes(n, "big") + x[0].to_bytes(n, "big")) if g2 else x.to_bytes(n, "big"))
        b[0] |= (0x80 if compressed_bit else 0) | (0x40 if inf else 0) | (0x20 if sign else 0)
    else:
        b = bytearray((x[0].to_bytes(n, "little") + x[1].to_bytes(n, "little")) if g2 else x.to_bytes(n, "little"))
        b[-1] |= (0x80 if sign else 0) | (0x40 if inf else 0)
    return bytes(b)


def sign_flag(name, enc):
    return bool(enc[0] & 0x20) if name == "bls12_381" else bool(enc[-1] & 0x80)


def rhs_of(G, x):
    return G.F.add(G.F.mul(G.F.sqr(x), x), G.b)


def norm_candidate(a, q):
    """which x0 candidate of the norm method yields the root of a (c1 != 0): 1 for (a0 + n) / 2, 2 for (a0 - n) / 2"""
    n = sqrt_fq((a[0] * a[0] + a[1] * a[1]) % q, q)
    assert n is not None
    inv2 = pow(2, q - 2, q)
    if sqrt_fq((a[0] + n) * inv2 % q, q):
        return 1
    assert sqrt_fq((a[0] - n) * inv2 % q, q)
    return 2


def real_rhs_points(G, q, want=2):
    """G2 points whose x^3 + b is real: 3 x0^2 x1 - x1^3 + Im b = 0 solved for x0 over a search in x1.  Returns
    (points with a square real part: the root is real, points with a non-square one: the root is purely imaginary)"""
    b0, b1 = G.b
    square, nonsquare = [], []
    x1 = 0
    while len(square) < want or len(nonsquare) < want:
        x1 += 1
        assert x1 < 4096, "no x with a real right-hand side found"
        x0 = sqrt_fq((x1**3 - b1) * pow(3 * x1, q - 2, q) % q, q)
        if not x0:
            continue
        for c in (x0, q - x0):
            x = (c, x1)
            a = rhs_of(G, x)
            assert a[1] == 0 and a[0] != 0
            y = sqrt_fq2(a, q)
            assert y is not None and G.on_curve((x, y))
            if y[1] == 0:
                assert y[0] * y[0] % q == a[0]
                square.append((x, y))
            else:
                assert y[0] == 0 and (q - y[1] * y[1]) % q == a[0]
                nonsquare.append((x, y))
    return square[:want], nonsquare[:want]


def build(name, g2):
    """[(label, encoding, status, affine point or None)] from the model alone"""
    cp = pm.CURVES[name]
    q = cp.q
    G = model_groups(cp)[g2]
    gen = cp.g2 if g2 else cp.g1
    rng = pm.SplitMix64(0xDEC0 + 2 * NAMES.index(name) + g2)
    out = [("identity", compress(name, g2, None), 1, None)]

    def valid(label, P):
        out.append((label, compress(name, g2, P), 1, P))

    members = [G.mul(gen, k) for k in [1, 2, cp.r - 1] + [rng.field(cp.r - 1) + 1 for _ in range(5)]]
    for i, P in enumerate(members):
        valid(f"member{i}", P)
    assert {sign_flag(name, compress(name, g2, P)) for P in members} == {False, True}, "members with each sign flag"
    valid("member3_neg", G.neg(members[3]))   # y and -y of one x
    assert sign_flag(name, out[-1][1]) != sign_flag(name, compress(name, g2, members[3]))
    randoms = [random_curve_point(G, cp, g2, rng) for _ in range(6)]
    assert any(G.mul(P, cp.r) is not None for P in randoms) or (name == "bn254" and not g2)   # whole-curve points, not members
    for i, P in enumerate(randoms):
        valid(f"random{i}", P)
    if g2:
        square, nonsquare = real_rhs_points(G, q)
        for i, P in enumerate(square):
            valid(f"real_rhs_square{i}", P)
            valid(f"real_rhs_square{i}_neg", G.neg(P))
        for i, P in enumerate(nonsquare):
            valid(f"real_rhs_nonsquare{i}", P)
            valid(f"real_rhs_nonsquare{i}_neg", G.neg(P))
        found = {1: 0, 2: 0}
        while min(found.values()) < 2:
            P = random_curve_point(G, cp, g2, rng)
            a = rhs_of(G, P[0])
            if a[1] == 0:
                continue
            k = norm_candidate(a, q)
            if found[k] < 2:
                valid(f"norm_candidate{k}_{found[k]}", P)
                found[k] += 1
    labels = [c[0] for c in out]
    if g2:
        for want in ("real_rhs_square0", "real_rhs_nonsquare0", "norm_candidate1_0", "norm_candidate2_0"):
            assert want in labels, want

    def invalid(label, enc):
        out.append((label, enc, 0, None))

    # an x with no point, and the encodings around it
    k = 1
    while True:
        k += 1
        x = (k, 1) if g2 else k
        if (sqrt_fq2(rhs_of(G, x), q) if g2 else sqrt_fq(rhs_of(G, x), q)) is None:
            break
    invalid("no_point", raw(name, g2, x))
    invalid("no_point_signed", raw(name, g2, x, sign=True))
    some = members[4][0]
    if g2:
        invalid("c0_eq_p", raw(name, g2, (q, some[1])))
        invalid("c0_eq_p_plus_1", raw(name, g2, (q + 1, some[1])))
        invalid("c1_eq_p", raw(name, g2, (some[0], q)))
        invalid("c1_eq_p_plus_1", raw(name, g2, (some[0], q + 1)))
        one = (1, 0)
    else:
        invalid("x_eq_p", raw(name, g2, q))
        invalid("x_eq_p_plus_1", raw(name, g2, q + 1))
        one = 1
    if name == "bls12_381":
        invalid("compressed_bit_clear", raw(name, g2, some, sign=sign_flag(name, compress(name, g2, members[4])), compressed_bit=False))
    invalid("infinity_with_x", raw(name, g2, one, inf=True))
    if g2:
        invalid("infinity_with_x_c1", raw(name, g2, (0, 1), inf=True))
    invalid("infinity_and_sign", raw(name, g2, (0, 0) if g2 else 0, inf=True, sign=True))
    assert all(len(c[1]) == enc_size(name, g2) for c in out)
    return out


@functools.lru_cache(maxsize=None)
def cases(name, g2):
    """build(), with each status held against g16_deserialize_points(compressed=1, validate=0) called one point at a time and each
    point against the model: (labels, encodings, uint8 status, (n, words) uint64 points -- the identity where the status is 0)"""
    g2 = bool(g2)
    built = build(name, g2)
    pts = to_arr([c[3] for c in built], name, g2)
    for (label, enc, status, P), want in zip(built, pts):
        try:
            got = deserialize_points(name, enc, 1, g2, compressed=True, validate=0)
        except g.binding.InvalidData:
            got = None
        assert (got is not None) == bool(status), label
        if status:
            assert got[0].tobytes() == want.tobytes(), label
            assert serialize_points(name, want, g2) == enc, label
    return [c[0] for c in built], [c[1] for c in built], np.array([c[2] for c in built], dtype=np.uint8), pts


def blob(encodings, idx=None):
    return b"".join(encodings if idx is None else [encodings[i] for i in idx])


def proofs_to_bytes(name, flat):
    """n x (A | B | C) affine -> n compressed proofs, the layout of proof_to_bytes(compressed=True)"""
    L = pm.CURVES[name].fq_limbs64
    flat = np.ascontiguousarray(flat, dtype=np.uint64).reshape(-1, 8 * L)
    n, fb = flat.shape[0], fq_bytes(name)
    out = np.zeros((n, 4 * fb), dtype=np.uint8)
    for lo, hi, g2, at in ((0, 2 * L, False, 0), (2 * L, 6 * L, True, fb), (6 * L, 8 * L, False, 3 * fb)):
        enc = serialize_points(name, np.ascontiguousarray(flat[:, lo:hi]), g2)
        out[:, at: at + enc_size(name, g2)] = np.frombuffer(enc, dtype=np.uint8).reshape(n, -1)
    return out
