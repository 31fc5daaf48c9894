"""Shared by the key-bytes tests (both tiers): per curve, group and encoding a labelled list of encoded points with what the big-int
model says of each -- whether the bytes decode, the point they name, and from those the status g16_decode_points owes them at every
validation level: 1 passed, 0 the bytes do not decode, 2 off the curve (uncompressed, validate >= 1), 3 outside the prime-order
subgroup (validate = 2).  The compressed lists are decompress_cases.build() plus the torsion points of subgroup_cases; the
uncompressed ones are written here from raw integers and explicit flag bits.  build() asserts its own labels against the model:
off-curve points are off the curve, torsion points are on it and outside the subgroup, BN254's G1 has no such point."""
import functools

import numpy as np

import decompress_cases as dc
import pymodel as pm
from subgroup_cases import NAMES, cases as subgroup_cases, cofactor, model_groups, random_curve_point, to_arr

VALIDATE = (0, 1, 2)


def enc_size(name, g2, compressed):
    return dc.enc_size(name, g2) * (1 if compressed else 2)


def larger(g2, y, q):
    """is y the larger of {y, -y}: canonical integers, Fq2 by c1 first, then c0"""
    if g2:
        if y[1] != (q - y[1]) % q:
            return y[1] > (q - y[1]) % q
        return y[0] > (q - y[0]) % q
    return y > (q - y) % q


def raw_xy(name, g2, x, y, inf=False, sign=False, compressed_bit=False):
    """an uncompressed encoding from raw integers (not reduced, so a coordinate >= p can be written) and explicit flag bits"""
    n = dc.fq_bytes(name)
    if name == "bls12_381":
        be = lambda v: v.to_bytes(n, "big")   # noqa: E731
        b = bytearray((be(x[1]) + be(x[0]) + be(y[1]) + be(y[0])) if g2 else be(x) + be(y))
        b[0] |= (0x80 if compressed_bit else 0) | (0x40 if inf else 0) | (0x20 if sign else 0)
    else:
        le = lambda v: v.to_bytes(n, "little")   # noqa: E731
        b = bytearray((le(x[0]) + le(x[1]) + le(y[0]) + le(y[1])) if g2 else le(x) + le(y))
        b[-1] |= (0x80 if sign else 0) | (0x40 if inf else 0)
    return bytes(b)


def write_xy(name, g2, P, q):
    """the encoding the writer gives a point: BN254 sets the sign flag of y, BLS12-381 has none in this form"""
    if P is None:
        zero = (0, 0) if g2 else 0
        return raw_xy(name, g2, zero, zero, inf=True)
    return raw_xy(name, g2, P[0], P[1], sign=name == "bn254" and larger(g2, P[1], q))


def build(name, g2, compressed):
    """[(label, encoding, decodes, point)]: point is None for the identity, else the (x, y) the bytes name -- on the curve or not"""
    cp = pm.CURVES[name]
    q = cp.q
    G = model_groups(cp)[g2]
    gen = cp.g2 if g2 else cp.g1
    _, torsion = subgroup_cases(name, g2)
    if cofactor(name, g2) == 1:
        assert name == "bn254" and not g2 and not torsion   # every point of BN254's G1 curve is in the subgroup: no such case exists
    else:
        assert torsion
    if compressed:
        out = [(label, enc, bool(status), P) for label, enc, status, P in dc.build(name, g2)]
        labels = [c[0] for c in out]
        assert "identity" in labels and "member0" in labels and "member3_neg" in labels   # the generator, both signs of one x
        assert out[labels.index("member0")][3] == gen
        out += [(f"order{l}", dc.compress(name, g2, T), True, T) for l, T in torsion.items()]
        return out
    rng = pm.SplitMix64(0xBE70 + 2 * NAMES.index(name) + g2)
    zero, one = ((0, 0), (1, 0)) if g2 else (0, 1)
    members = [G.mul(gen, k) for k in [1, 2, cp.r - 1] + [rng.field(cp.r - 1) + 1 for _ in range(3)]]
    out = [("identity", write_xy(name, g2, None, q), True, None)]
    for i, P in enumerate(members):
        out.append((f"member{i}", write_xy(name, g2, P, q), True, P))
    out.append(("member3_neg", write_xy(name, g2, G.neg(members[3]), q), True, G.neg(members[3])))
    for i in range(4):
        P = random_curve_point(G, cp, g2, rng)
        out.append((f"random{i}", write_xy(name, g2, P, q), True, P))
    for l, T in torsion.items():   # on the curve, outside the subgroup
        out.append((f"order{l}", write_xy(name, g2, T, q), True, T))
    some = members[4]
    off = (some[0], G.F.add(some[1], G.F.one))
    out.append(("off_curve", write_xy(name, g2, off, q), True, off))
    out.append(("zero_without_flag", raw_xy(name, g2, zero, zero), True, (zero, zero)))   # the identity's limbs, but a finite point off the curve
    if name == "bn254":
        sign = larger(g2, some[1], q)
        out.append(("wrong_sign_flag", raw_xy(name, g2, some[0], some[1], sign=not sign), True, some))   # not re-checked, as on the host
        out.append(("infinity_and_sign", raw_xy(name, g2, zero, zero, inf=True, sign=True), False, None))
    else:
        out.append(("compressed_bit_set", raw_xy(name, g2, some[0], some[1], compressed_bit=True), False, None))
        out.append(("sign_bit_set", raw_xy(name, g2, some[0], some[1], sign=True), False, None))
        out.append(("infinity_and_sign", raw_xy(name, g2, zero, zero, inf=True, sign=True), False, None))
    bn_sign = lambda y: name == "bn254" and larger(g2, y, q)   # noqa: E731
    if g2:
        for k in range(2):
            for what, v in (("eq_p", q), ("eq_p_plus_1", q + 1)):
                x = tuple(v if j == k else some[0][j] for j in range(2))
                y = tuple(v if j == k else some[1][j] for j in range(2))
                out.append((f"x_c{k}_{what}", raw_xy(name, g2, x, some[1], sign=bn_sign(some[1])), False, None))
                out.append((f"y_c{k}_{what}", raw_xy(name, g2, some[0], y), False, None))
        out.append(("infinity_with_y_c1", raw_xy(name, g2, zero, (0, 1), inf=True), False, None))
    else:
        for what, v in (("eq_p", q), ("eq_p_plus_1", q + 1)):
            out.append((f"x_{what}", raw_xy(name, g2, v, some[1], sign=bn_sign(some[1])), False, None))
            out.append((f"y_{what}", raw_xy(name, g2, some[0], v), False, None))
    out.append(("infinity_with_y", raw_xy(name, g2, zero, one, inf=True), False, None))
    out.append(("infinity_with_x", raw_xy(name, g2, one, zero, inf=True), False, None))
    assert all(len(c[1]) == enc_size(name, g2, False) for c in out)
    return out


def model_status(G, cp, compressed, decodes, P, validate, member):
    """the status byte from the model alone; member: is [r]P the identity (computed once per point)"""
    if not decodes:
        return 0
    if P is None:
        return 1
    if not compressed and validate >= 1 and not G.on_curve(P):
        return 2
    if validate >= 2 and not member:
        return 3
    return 1


@functools.lru_cache(maxsize=None)
def cases(name, g2, compressed):
    """(labels, encodings, {validate: uint8 statuses}, {validate: (n, words) uint64 points -- the identity unless the status is 1})"""
    g2, compressed = bool(g2), bool(compressed)
    cp = pm.CURVES[name]
    G = model_groups(cp)[g2]
    built = build(name, g2, compressed)
    member = [P is None or (G.on_curve(P) and G.mul(P, cp.r) is None) for _, _, _, P in built]
    status, points = {}, {}
    for v in VALIDATE:
        st = [model_status(G, cp, compressed, d, P, v, m) for (_, _, d, P), m in zip(built, member)]
        status[v] = np.array(st, dtype=np.uint8)
        points[v] = to_arr([P if s == 1 and P is not None and not _is_zero(P, g2) else None for (_, _, _, P), s in zip(built, st)], name, g2)
    labels = [c[0] for c in built]
    # the labels the issue names, held against the model
    for label, (_, _, d, P), m in zip(labels, built, member):
        if label.startswith("order"):
            assert d and G.on_curve(P) and not m, label
        if label in ("off_curve", "zero_without_flag"):
            assert d and not G.on_curve(P), label
        if label.startswith("member") or label == "wrong_sign_flag":
            assert d and m, label
    if not compressed:
        assert status[1][labels.index("off_curve")] == 2 and status[0][labels.index("off_curve")] == 1
    return labels, [c[1] for c in built], status, points


def _is_zero(P, g2):
    return P == ((0, 0), (0, 0)) if g2 else P == (0, 0)


def blob(encodings, idx=None):
    return b"".join(encodings if idx is None else [encodings[i] for i in idx])


# ---- the container (a serialized ProvingKey, src/data_structures.rs:31-44, 125-143) ----------------------------------------------
SECTIONS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "beta_g1", "delta_g1", "a_query", "b_g1_query", "b_g2_query", "h_query",
            "l_query")
VECS = ("gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")
G2_SECTIONS = ("beta_g2", "gamma_g2", "delta_g2", "b_g2_query")


def section_offsets(name, ck, compressed):
    """{section: (offset of its length word or first point, offset of its first point, bytes per point, count)} by the file's layout"""
    L = pm.CURVES[name].fq_limbs64 * 8
    g1s, g2s = (L, 2 * L) if compressed else (2 * L, 4 * L)
    n, nv, ni = ck.domain_size, ck.num_vars, ck.num_inputs
    counts = dict(alpha_g1=1, beta_g2=1, gamma_g2=1, delta_g2=1, gamma_abc_g1=ni, beta_g1=1, delta_g1=1, a_query=nv, b_g1_query=nv,
                  b_g2_query=nv, h_query=n - 1, l_query=nv - ni)
    out, pos = {}, 0
    for sec in SECTIONS:
        size = g2s if sec in G2_SECTIONS else g1s
        first = pos + (8 if sec in VECS else 0)
        out[sec] = (pos, first, size, counts[sec])
        pos = first + counts[sec] * size
    return out, pos
