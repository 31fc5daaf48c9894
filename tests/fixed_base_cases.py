"""Cases for the fixed-base kernels in place (TEST INFRASTRUCTURE, no GPU): fixed_base_table_kernel and fixed_base_mul_kernel of
csrc/setup.hip through the public entry points alone, srs_from_trapdoor and generate_parameters_with_qap.  table[w * 255 + d - 1] =
d * 2^(8 w) * G; a scalar's canonical bytes pick one entry per non-zero byte.  Expected values are pymodel's k G with k reduced mod r
by the model (cached per curve, group and k); the generators are srs_cases.secrets', a non-standard pair.
Every property a case is named after is asserted here with the model alone."""
import functools
import random

import pymodel as pm
import srs_cases as sc

WINDOWS, DIGITS = 32, 255
DIGIT_SEED = "fixed-base/digits"


@functools.lru_cache(maxsize=None)
def gens(curve):
    s = sc.secrets(pm.CURVES[curve])
    cp = pm.CURVES[curve]
    assert s["g1"] != cp.g1 and s["g2"] != cp.g2
    return s["g1"], s["g2"]


@functools.lru_cache(maxsize=None)
def multiple(curve, g2, k):
    """(k mod r) G, None for the identity"""
    cp = pm.CURVES[curve]
    k %= cp.r
    return pm.groups(cp)[g2].mul(gens(curve)[g2], k) if k else None


def window_bytes(k):
    return [(k >> (8 * w)) & 0xFF for w in range(WINDOWS)]


def table_entries(k):
    """the table indices a canonical scalar reads"""
    return [w * DIGITS + d - 1 for w, d in enumerate(window_bytes(k)) if d]


def single_scalars(curve):
    """[(name, k)] for srs_from_trapdoor(n = 1, tau = 1, alpha, beta): every k below r"""
    r = pm.CURVES[curve].r
    top = r >> 248
    ones = ((top - 1) << 248) | ((1 << 248) - 1)        # every byte 255 as far as that stays below r: the low 31, the top one r's - 1
    assert ones < r and window_bytes(ones)[:31] == [255] * 31
    out = [("0", 0), ("1", 1), ("2", 2), ("255", 255), ("256", 256), ("r - 1", r - 1), ("(r - 1) / 2", (r - 1) // 2), ("(r + 1) / 2", (r + 1) // 2),
           ("every byte 255 below r", ones), ("31 bytes 255", (1 << 248) - 1), ("the largest k below r", r - 1)]
    rng = random.Random("fixed-base/single/%s" % curve)
    for w in range(WINDOWS):
        d = rng.randrange(1, 256) if w < 31 else rng.randrange(1, top)
        k = d << (8 * w)
        assert k < r and table_entries(k) == [w * DIGITS + d - 1]
        out.append(("one non-zero byte, position %d" % w, k))
    out.append(("byte 255 at position 0", 255))
    out.append(("the top byte alone at r's - 1", (top - 1) << 248))
    assert table_entries(0) == [] and table_entries(1) == [0] and table_entries(256) == [DIGITS] and len(table_entries(ones)) == 32
    assert all(0 <= k < r for _, k in out)
    return out


def digits():
    rng = random.Random(DIGIT_SEED)
    return [1, 2, 3, 127, 128, 254, 255] + [rng.randrange(1, 256) for _ in range(8)]


def window_cases(curve):
    """[(d, d')] for srs_from_trapdoor(n = 32, tau = 256, alpha = d, beta = d'): alpha_tau_g1[w] = d 256^w G.  Asserts that for w < 31
    the scalar's only non-zero byte is d at position w (so the output IS table[w * 255 + d - 1], and tau_g2[w] is table[w * 255] of G2),
    and that in window 31 some products wrap mod r and read several entries"""
    r = pm.CURVES[curve].r
    ds = digits()
    wrapped = 0
    for d in ds:
        for w in range(WINDOWS):
            k = d * pow(256, w, r) % r
            if w < 31:
                assert k == d << (8 * w) and table_entries(k) == [w * DIGITS + d - 1]
            elif d << 248 >= r:
                assert k != d << 248 and len(table_entries(k)) > 1
                wrapped += 1
    assert wrapped >= 4 and (1 << 248) < r                 # d = 1 never wraps: tau_g2[31] is table[31 * 255]
    for i in range(32, 63):                                # tau_g1 goes on to 256^62: every power past 31 is reduced
        assert pow(256, i, r) != 1 << (8 * i)
    return list(zip(ds, ds[5:] + ds[:5]))


def expected_srs(curve, n, tau, alpha, beta):
    r = pm.CURVES[curve].r
    pw = [pow(tau, i, r) for i in range(2 * n - 1)]
    return dict(tau_g1=[multiple(curve, 0, s) for s in pw], tau_g2=[multiple(curve, 1, s) for s in pw[:n]],
                alpha_tau_g1=[multiple(curve, 0, alpha * s) for s in pw[:n]], beta_tau_g1=[multiple(curve, 0, beta * s) for s in pw[:n]],
                beta_g2=[multiple(curve, 1, beta)])


SIZES = (1, 32, 33, 63, 64, 65)   # n; the three scalar arrays hold n, n and 2 n - 1 entries


def size_cases(curve):
    """[(n, tau, alpha, beta, what)]: array lengths 1, 63, 64, 65 and 127 among n and 2 n - 1, with a zero scalar (tau = 0: every power
    but the first is the identity) and with tau = r - 1 (alternating +-G)"""
    r = pm.CURVES[curve].r
    lens = {n for n in SIZES} | {2 * n - 1 for n in SIZES}
    assert {1, 63, 64, 65, 127} <= lens
    rng = random.Random("fixed-base/sizes/%s" % curve)
    out = []
    for n in SIZES:
        a, b = rng.randrange(1, r), rng.randrange(1, r)
        out.append((n, 0, a, b, "tau = 0"))
        out.append((n, r - 1, a, b, "tau = r - 1"))
    e = expected_srs(curve, 3, 0, 5, 7)
    assert e["tau_g1"][1:] == [None] * 4 and e["tau_g1"][0] == gens(curve)[0] and e["alpha_tau_g1"][1:] == [None, None]
    e = expected_srs(curve, 3, r - 1, 1, 1)
    G1 = pm.groups(pm.CURVES[curve])[0]
    assert e["tau_g1"] == [gens(curve)[0], G1.neg(gens(curve)[0])] * 2 + [gens(curve)[0]]
    return out


def qap_targets(curve):
    r = pm.CURVES[curve].r
    top = r >> 248
    return [0, 1, r - 1, ((top - 1) << 248) | ((1 << 248) - 1)]


def qap_circuit(curve, t, num_witness=None):
    """A crafted R1CS whose witness column j has ONE entry, in row j of A and of B, with the coefficient target_j * u_j(t)^-1: then
    a_query[ni + j] = b_g1_query[ni + j] = target_j G1 and b_g2_query[ni + j] = target_j G2.  The last witness variable is unused
    (no entry anywhere).  num_witness = 0: l_query is empty; 1: a single entry.  Returns (R1CS, {column: target})."""
    cp = pm.CURVES[curve]
    r = cp.r
    tg = qap_targets(curve)
    nw = len(tg) + 1 if num_witness is None else num_witness
    ni, nc = 1, 6
    u = pm.Domain(cp, nc + ni).lagrange_at(t)
    assert pm.Domain(cp, nc + ni).vanishing(t) != 0 and all(x for x in u)
    a, b, c = [[] for _ in range(nc)], [[] for _ in range(nc)], [[] for _ in range(nc)]
    want = {}
    for j in range(min(nw, len(tg))):
        cf = tg[j] * pow(u[j], r - 2, r) % r
        a[j].append((cf, ni + j))
        b[j].append((cf, ni + j))
        want[ni + j] = tg[j]
    b[5].append((1, 0))                                    # something on the constant's column too
    c[5].append((3, 0))
    cs = pm.R1CS(ni, nw, a, b, c)
    av, bv, cv, zt, m, n = pm.instance_map_with_evaluation(cp, cs, t)
    for col, target in want.items():
        assert av[col] == bv[col] == target, (col, target)
    if num_witness is None:
        assert av[ni + len(tg)] == bv[ni + len(tg)] == cv[ni + len(tg)] == 0     # the unused variable
        assert any(cf == 0 for row in a for cf, _ in row)                         # target 0: an explicit zero coefficient
    assert len(av) == ni + nw
    return cs, want
