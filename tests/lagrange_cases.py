"""The Lagrange form of an SRS: the cases the CPU and GPU tiers share (TEST INFRASTRUCTURE, no GPU), built on table_cases.py,
phase1_cases.py and srs_cases.py.

The transform.  model_transform() runs the Gentleman-Sande stages of g16_group_ntt_windowed literally in table_cases.Model -- the
plain affine law on any (x, y), no reduction modulo a group order -- and reports which case of the law every butterfly's sum and
difference met (ADD, DBL, ZERO, TAKE_P, TAKE_Q), so that test_lagrange_cases.py can assert that each edge input meets the collision
it is named after.  A twiddle w multiplies as the library does: min(w, r - w) times the point, negated when r - w was taken.  For a
point outside the prime-order subgroup that is not w times the point (r P is not the identity); plain=True multiplies by w itself,
so that the premise "the rule matters on these inputs" can be asserted too.

edge_inputs() lists the arrays: identities, identities between points, a constant array, P and -P in turn, the multiples of P, the
multiples of a point of order two, three and (G2) four from table_cases.point_classes -- each on its own curve y^2 = x^3 + b', where
the law is still a group law -- and, on BLS12-381 G1, k G + T with T = (0, 2) of order three ON the curve: points of order 3 r."""
import functools

import numpy as np

import phase1_cases as pc
import pymodel as pm
import table_cases as tc

LOG_NS = (3, 6)


def bitrev(i: int, bits: int) -> int:
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def twiddle_mul(curve: str, g2: bool, P, w: int, plain: bool = False):
    r = pm.CURVES[curve].r
    w %= r
    if plain or w <= r - w:
        return pc.expected(curve, g2, P, w)
    return tc.model(curve, g2).neg(pc.expected(curve, g2, P, r - w))


def model_transform(curve: str, g2: bool, pts, inverse: bool, seen=None, plain: bool = False):
    """natural order in and out; seen: a set that receives (stage, 'sum' | 'diff', kind) of every butterfly"""
    m = tc.model(curve, g2)
    cp = pm.CURVES[curve]
    r, n = cp.r, len(pts)
    log_n = n.bit_length() - 1
    assert n == 1 << log_n
    if n == 1:
        return list(pts)
    dom = pm.Domain(cp, n)
    root, scale = (dom.omega_inv, dom.n_inv) if inverse else (dom.omega, 1)
    d = list(pts)
    for s in range(log_n):
        half = n >> (s + 1)
        for t in range(n // 2):
            k = t % half
            i = (t // half) * 2 * half + k
            a, b = d[i], d[i + half]
            if seen is not None:
                seen.add((s, "sum", m.kind(a, b)))
                seen.add((s, "diff", m.kind(a, m.neg(b))))
            S, D = m.add(a, b), m.add(a, m.neg(b))
            e = k << s
            if inverse and s == 0:
                S = twiddle_mul(curve, g2, S, scale, plain)
                D = twiddle_mul(curve, g2, D, pow(root, e, r) * scale, plain)
            elif e:
                D = twiddle_mul(curve, g2, D, pow(root, e, r), plain)
            d[i], d[i + half] = S, D
    return [d[bitrev(i, log_n)] for i in range(n)]


def to_array(curve: str, g2: bool, pts) -> np.ndarray:
    m = tc.model(curve, g2)
    return np.array([tc.abi_words(m, P) for P in pts], dtype=np.uint64)


def multiples(curve: str, g2: bool, P, count: int):
    """[P, 2 P, ..., count P] by repeated addition in the model"""
    m = tc.model(curve, g2)
    out = [P]
    while len(out) < count:
        out.append(m.add(out[-1], P))
    return out


@functools.lru_cache(maxsize=None)
def edge_inputs(curve: str, g2: bool, log_n: int):
    """[(label, points)], n = 2^log_n points each"""
    m = tc.model(curve, g2)
    n = 1 << log_n
    cls = dict(tc.point_classes(curve, g2))
    gen = multiples(curve, g2, m.gen, n + 2)
    P = gen[4]
    out = [("identities", [None] * n),
           ("identities between points", [gen[i] if i % 2 else None for i in range(n)]),
           ("points between identities", [None if i % 4 == 3 else gen[i] for i in range(n)]),
           ("constant", [P] * n),
           ("P, -P in turn", [P if i % 2 == 0 else m.neg(P) for i in range(n)]),
           ("multiples of P", multiples(curve, g2, P, n))]
    two = cls["(x, 0)"][0]
    out.append(("order two, constant", [two] * n))
    out.append(("order two between identities", [two if i % 3 else None for i in range(n)]))
    three = cls["(0, y)"][0]
    out.append(("multiples of a point of order three", multiples(curve, g2, three, n)))
    if g2:
        out.append(("multiples of a point of order four", multiples(curve, g2, cls["order 4"][0], n)))
    for j, Q in enumerate(pc.small_order_points(curve, g2)):
        out.append(("small order %d and its negative" % j, [Q if (i * i + j) % 3 else m.neg(Q) for i in range(n)]))
    if curve == "bls12_381" and not g2:
        T = (0, 2)
        assert T in cls["(0, y)"] and pm.groups(pm.CURVES[curve])[0].on_curve(T)
        out.append(("k G + T, order 3 r on the curve", [m.add(gen[i], T) for i in range(n)]))
    for label, pts in out:
        assert len(pts) == n, label
    return out


def edge_ids(curve: str, g2: bool):
    return [label for label, _ in edge_inputs(curve, g2, LOG_NS[0])]
