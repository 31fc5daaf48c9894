"""Shared by the transform edge tests (both tiers): named worst-case vectors over Fr and a circuit whose witness map transforms
three ARBITRARY vectors (TEST INFRASTRUCTURE).

The NTT kernels (csrc/ntt.hip) never reduce inside a pass: sums stay lazy for up to ten stages, the DIF subtraction adds a
redundant multiple of p chosen from a stage counter, the stage-0 twiddle product is skipped, and the tile is folded back once
at the end.  All of that is correct only while the data stays under a bound, and uniform random data sits near HALF of the
only bound that accumulates (the all-sums chain, element 0 of a DIF tile).  The vectors here put the chains at their real
ceilings and produce lazy values that are exact multiples of p:

  zeros / ones / const_pm1        constant 0, 1, p - 1: the all-sums chain reaches 2^K (p - 1), every other output is k p
  impulse_first / _mid / _last    p - 1 at one index: every butterfly sees one zero operand
  alt_pm1_0 / alt_pm1_1           p - 1 at even indices, 0 (1) at odd: pairs cancel to exactly p
  half_pm1                        first half p - 1, second half 0
  alt_0_pm1 / half_0_pm1          the mirror images: the SUBTRAHEND chain of a DIF difference u - v + 2^(k+1) p is the heavy one
                                  (v = 2^k (p - 1) against u = 0 is the floor of that expression; the vectors above have u >= v)
  geometric_1 / geometric_h       x[i] = w^(-j i), j = 1 and n/2 + 1: the forward transform is n at index j and an exact zero
                                  elsewhere, reached through non-trivial twiddles
  rand_edges                      rand with one entry of every eight replaced by 0, 1 or p - 1
  rand                            SplitMix64 field elements (what oracle.rand_fr gives for the same seed)

Everything is generated; nothing here reads a file.  Integers are canonical; arrays are the 4 x 64-bit Montgomery limbs the C
ABIs take."""
import numpy as np

import pymodel as pm
from helpers import Csr, FlatCircuit

CURVES = {"bls12_381": pm.BLS12_381, "bn254": pm.BN254}
NAMES = ["zeros", "ones", "const_pm1", "impulse_first", "impulse_mid", "impulse_last", "alt_pm1_0", "alt_pm1_1", "half_pm1",
         "alt_0_pm1", "half_0_pm1", "geometric_1", "geometric_h", "rand_edges", "rand"]
MODES = [(False, False), (True, False), (False, True), (True, True)]   # (inverse, coset)
R = 1 << 256


def geometric_index(name, n):
    """j of geometric_<..>, reduced mod n (n = 2: n/2 + 1 = 0 mod n, the constant-one vector)"""
    return (1 if name == "geometric_1" else n // 2 + 1) % n


def to_mont(vals, p):
    """canonical ints -> uint64[len, 4] Montgomery (helpers.ints_to_mont without its per-limb Python loop)"""
    buf = b"".join((v * R % p).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def from_mont(arr, p):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    rinv = pow(R, p - 2, p)
    return [int.from_bytes(raw[i:i + 32], "little") * rinv % p for i in range(0, len(raw), 32)]


def _edge_plan(length, seed):
    """rand_edges: (index, which of 0 / 1 / p - 1) for one entry of every block of eight"""
    rng = np.random.RandomState(1000 + seed)
    nblk = (length + 7) // 8
    pos = np.arange(nblk) * 8 + rng.randint(0, 8, nblk)
    keep = pos < length
    return pos[keep], rng.randint(0, 3, nblk)[keep]


def _pattern(name, n, length):
    """structured vectors as (values, index array): entry values[index[i]] at position i"""
    idx = np.zeros(length, dtype=np.int64)
    i = np.arange(length)
    if name == "zeros":
        return "0", idx
    if name == "ones":
        return "1", idx
    if name == "const_pm1":
        return "m", idx
    if name.startswith("impulse_"):
        idx[{"first": 0, "mid": length // 2, "last": length - 1}[name[8:]]] = 1
        return "0m", idx
    if name == "alt_pm1_0":
        return "m0", i & 1
    if name == "alt_pm1_1":
        return "m1", i & 1
    if name == "alt_0_pm1":
        return "0m", i & 1
    if name == "half_pm1":
        return "m0", (i >= (length + 1) // 2).astype(np.int64)
    if name == "half_0_pm1":
        return "0m", (i >= (length + 1) // 2).astype(np.int64)
    return None


def vector_ints(cp, name, n, seed=0, length=None):
    """the named vector as canonical ints: `length` entries (default n) of the vector defined for the n-point domain"""
    p = cp.r
    length = n if length is None else length
    pat = _pattern(name, n, length)
    if pat is not None:
        table = [{"0": 0, "1": 1, "m": p - 1}[c] for c in pat[0]]
        return [table[k] for k in pat[1]]
    if name.startswith("geometric_"):
        dom = pm.Domain(cp, n)
        step = pow(dom.omega_inv, geometric_index(name, n), p)
        out, t = [], 1
        for _ in range(length):
            out.append(t)
            t = t * step % p
        return out
    rng = pm.SplitMix64(seed)
    out = [rng.field(p) for _ in range(length)]
    if name == "rand_edges":
        for k, w in zip(*_edge_plan(length, seed)):
            out[k] = (0, 1, p - 1)[w]
    else:
        assert name == "rand", name
    return out


def vector_mont(cp, name, n, seed=0, length=None, orc=None):
    """the same vector as uint64[length, 4] Montgomery.  With an oracle the random part comes from oracle.rand_fr (the same
    SplitMix64 stream, test_transform_cases pins the two against each other) and nothing loops over the entries in Python but the
    geometric progression, so 2^19 entries cost well under a second."""
    p = cp.r
    length = n if length is None else length
    pat = _pattern(name, n, length)
    if pat is not None:
        table = to_mont([{"0": 0, "1": 1, "m": p - 1}[c] for c in pat[0]], p)
        return np.ascontiguousarray(table[pat[1]])
    if name in ("rand", "rand_edges") and orc is not None:
        out = orc.rand_fr(cp.name, seed, length)
        if name == "rand_edges":
            pos, which = _edge_plan(length, seed)
            out[pos] = to_mont([0, 1, p - 1], p)[which]
        return out
    return to_mont(vector_ints(cp, name, n, seed, length), p)


# ---------------------------------------------------------------------------------------------------------------------------
# triples (va, vb, vc) for free_vector_circuit: (name, seed) each; "product" = va .* vb (the one satisfied system)
# ---------------------------------------------------------------------------------------------------------------------------
TRIPLES = {
    "pm1_all": (("const_pm1", 0), ("const_pm1", 0), ("const_pm1", 0)),
    "pm1_pm1_zeros": (("const_pm1", 0), ("const_pm1", 0), ("zeros", 0)),
    "zeros_rand_rand": (("zeros", 0), ("rand", 21), ("rand", 22)),
    "alt_alt_pm1": (("alt_pm1_1", 0), ("alt_pm1_0", 0), ("const_pm1", 0)),
    "mirror_alt_half_pm1": (("alt_0_pm1", 0), ("half_0_pm1", 0), ("half_pm1", 0)),
    "impulses": (("impulse_first", 0), ("impulse_mid", 0), ("impulse_last", 0)),
    "ones_pm1_zeros": (("ones", 0), ("const_pm1", 0), ("zeros", 0)),   # a = 1 everywhere: the DIT half of the fused kernel at 1 + 2 K p
    "geometric": (("geometric_1", 0), ("geometric_h", 0), ("geometric_1", 0)),
    "rand_edges": (("rand_edges", 31), ("rand_edges", 32), ("rand_edges", 33)),
    "satisfied": (("rand", 41), ("rand", 42), ("product", 0)),
    "rand": (("rand", 51), ("rand", 52), ("rand", 53)),
}
TRIPLES_AT_19 = ["rand", "pm1_all", "geometric", "satisfied"]   # see test_gpu_transform_edges: the oracle's time at k = 19


def triple_mont(cp, k, tname, orc=None):
    """the three vectors of a triple, nc = 2^k - 1 Montgomery entries each"""
    n, p = 1 << k, cp.r
    nc = n - 1
    out, made = [], {}
    for name, seed in TRIPLES[tname]:
        if name == "product":   # on the Montgomery forms: (x R)(y R) / R
            rinv = pow(R, p - 2, p)
            ra, rb = (np.ascontiguousarray(v, dtype="<u8").tobytes() for v in out[:2])
            buf = b"".join((int.from_bytes(ra[i:i + 32], "little") * int.from_bytes(rb[i:i + 32], "little") % p * rinv % p).to_bytes(32, "little")
                           for i in range(0, len(ra), 32))
            out.append(np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64))
        else:
            if (name, seed) not in made:
                made[name, seed] = vector_mont(cp, name, n, seed, nc, orc)
            out.append(made[name, seed].copy())
    return out


def free_vector_circuit(curve, k, va, vb, vc, coeff=1):
    """FlatCircuit with num_inputs = 1, nc = 2^k - 1 constraints and z = [1] + va + vb + vc (Montgomery uint64[nc, 4] each): row i of
    A, B, C is the single term coeff * z[1 + i], coeff * z[1 + nc + i], coeff * z[1 + 2 nc + i].  The witness map therefore
    transforms a = coeff va || 1, b = coeff vb || 0, c = coeff vc || 0 -- three arbitrary vectors; the system need not be
    satisfied, (a b - c) / Z is computed on the coset either way.  The CSR arrays are built in numpy (no row lists)."""
    cp = CURVES[curve]
    nc = (1 << k) - 1
    assert va.shape == vb.shape == vc.shape == (nc, 4)
    z = np.ascontiguousarray(np.concatenate([to_mont([1], cp.r), va, vb, vc]), dtype=np.uint64)
    val = np.ascontiguousarray(np.tile(to_mont([coeff % cp.r], cp.r), (nc, 1)))
    row_ptr = np.arange(nc + 1, dtype=np.uint64)
    abc = [Csr(row_ptr, np.arange(1 + m * nc, 1 + (m + 1) * nc, dtype=np.uint32), val) for m in range(3)]
    return FlatCircuit(curve, 1, nc, 1 + 3 * nc, abc, z)


def r1cs_of(ck):
    """a FlatCircuit's CSR arrays and assignment back as the big-int model's (R1CS, z): what pymodel.witness_map_from_matrices
    takes.  Small circuits only (Python loops)."""
    p = CURVES[ck.curve].r
    mats = []
    for m in ck.abc:
        vals = from_mont(m.val, p)
        mats.append([[(vals[t], int(m.col[t])) for t in range(int(m.row_ptr[i]), int(m.row_ptr[i + 1]))]
                     for i in range(ck.num_constraints)])
    return pm.R1CS(ck.num_inputs, ck.num_vars - ck.num_inputs, *mats), from_mont(ck.z, p)
