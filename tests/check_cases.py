"""Cases of the R1CS satisfaction check, shared by the CPU tier (test_r1cs_check_host.py) and the GPU tier (test_gpu_r1cs_check.py).
TEST INFRASTRUCTURE: not imported by the product.

A base circuit (in the style of random_circuit in test_gpu_circom.py) has nc constraints over ni instance variables: A and B rows of
0 - 3 terms with coefficients 1, p - 1 and random ones (row i % 5 == 3 of A and row i % 7 == 2 of B are empty), and C row i is ONE
dedicated witness variable holding a_i b_i that no other row references -- so adding a delta to that variable breaks row i and only
row i.  A case is a base circuit plus a set of rows broken that way.  The base (rows, assignment, limb arrays and the per-row sums of
A and B, which no case changes) is built once per (curve, nc, ni) and shared; a case only rewrites the dedicated variables of its rows.

What a case EXPECTS comes from oracle/pymodel.py (evaluate_constraint), never from the code under test."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import pymodel as pm
from helpers import FlatCircuit, circuit_from_pymodel, ints_to_mont

CURVES = ["bls12_381", "bn254"]
CP = pm.CURVES
# one lane, a wave edge, a block edge, several blocks, many blocks contending on the two atomics
NCS = [0, 1, 63, 64, 65, 255, 256, 257, 1000, (1 << 16) + 1]
NIS = [1, 2]


def deltas(p: int) -> List[int]:
    """cycled over a case's bad rows: +1, -1, +2^224, +2^32 -- off by the lowest limb only, or by one high limb only"""
    return [1, p - 1, (1 << 224) % p, (1 << 32) % p]


@dataclass
class Base:
    cp: "pm.CurveParams"
    nc: int
    ni: int
    cs: "pm.R1CS"
    z: List[int]
    ck: FlatCircuit          # limb arrays of the matrices and of the satisfying assignment
    a: List[int]             # <A_i, z>, <B_i, z>: rows of A and B never reference a dedicated variable (asserted below)
    b: List[int]
    c0: int                  # column of row 0's dedicated variable; row i's is c0 + i

    def matrices(self, g):
        """one ConstraintMatrices per base and process (a prover caches its device copy by the object's identity)"""
        if getattr(self, "_mats", None) is None:
            ck = self.ck
            self._mats = g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints,
                                              *[(m.row_ptr, m.col, m.val) for m in ck.abc])
        return self._mats


@functools.lru_cache(maxsize=None)
def base(curve: str, nc: int, ni: int) -> Base:
    cp = CP[curve]
    p = cp.r
    rng = pm.SplitMix64(7919 * nc + 31 * ni + len(curve))
    z = [1] + [rng.field(p) for _ in range(ni - 1 + nc + 3)]
    nfree = len(z)

    def row(skip):
        if skip:
            return []
        out = []
        for _ in range(1 + rng.next() % 3):
            cf = (1, p - 1, rng.field(p), rng.field(p))[rng.next() % 4]
            out.append((cf, rng.next() % nfree))
        return out

    A = [row(i % 5 == 3) for i in range(nc)]
    B = [row(i % 7 == 2) for i in range(nc)]
    a = [pm.evaluate_constraint(r, z, p) for r in A]
    b = [pm.evaluate_constraint(r, z, p) for r in B]
    Cm = [[(1, nfree + i)] for i in range(nc)]
    z = z + [x * y % p for x, y in zip(a, b)]
    assert all(col < nfree for r in A + B for _, col in r)
    cs = pm.R1CS(ni, len(z) - ni, A, B, Cm)
    return Base(cp, nc, ni, cs, z, circuit_from_pymodel(cp, cs, z), a, b, nfree)


def bad_sets(nc: int) -> List[Tuple[str, List[int]]]:
    """each set at every nc that can hold it"""
    out: List[Tuple[str, List[int]]] = [("none", [])]
    if nc >= 1:
        out += [("first", [0]), ("last", [nc - 1])]
    if nc >= 65:
        out.append(("wave_edge", [63, 64]))
    if nc >= 257:
        out.append(("block_edge", [255, 256]))
    if nc >= 1:
        out.append(("every", list(range(nc))))
        rng = pm.SplitMix64(1000003 + nc)
        out.append(("random_1pct", sorted({rng.next() % nc for _ in range(max(1, nc // 100))})))
    return out


@dataclass
class Expected:
    """what pymodel says: how many rows fail, the first of them, its three sums (integers mod p)"""
    n_unsatisfied: int
    first_row: Optional[int]
    abc: Optional[Tuple[int, int, int]]


@dataclass
class Case:
    base: Base
    name: str
    z: np.ndarray            # (num_vars, 4) Montgomery limbs
    expected: Expected


def expect(cs: "pm.R1CS", z: List[int], p: int, a: Optional[List[int]] = None, b: Optional[List[int]] = None) -> Expected:
    """the model's verdict row by row; a, b: sums of A and B already known for this assignment"""
    bad, first = 0, None
    for i in range(cs.num_constraints):
        ai = a[i] if a is not None else pm.evaluate_constraint(cs.a[i], z, p)
        bi = b[i] if b is not None else pm.evaluate_constraint(cs.b[i], z, p)
        ci = pm.evaluate_constraint(cs.c[i], z, p)
        if ai * bi % p != ci:
            bad += 1
            if first is None:
                first = (i, (ai, bi, ci))
    if cs.num_constraints <= 4096:   # (the big-int loop twice only where it is cheap)
        assert (bad == 0) == pm.is_satisfied(cs, z, p)
    return Expected(bad, first[0] if first else None, first[1] if first else None)


def case(curve: str, nc: int, ni: int, name: str) -> Case:
    bs = base(curve, nc, ni)
    p = bs.cp.r
    rows = dict(bad_sets(nc))[name]
    z = list(bs.z)
    zm = bs.ck.z.copy()
    ds = deltas(p)
    for k, i in enumerate(rows):
        z[bs.c0 + i] = (z[bs.c0 + i] + ds[k % 4]) % p
    if rows:
        zm[[bs.c0 + i for i in rows]] = ints_to_mont([z[bs.c0 + i] for i in rows], p, 4)
    ex = expect(bs.cs, z, p, bs.a, bs.b)
    assert ex.n_unsatisfied == len(rows) and ex.first_row == (rows[0] if rows else None)
    return Case(bs, name, zm, ex)


# ---- fixed rows ----------------------------------------------------------------------------------------------------------------
@dataclass
class FixedCase:
    cp: "pm.CurveParams"
    name: str
    cs: "pm.R1CS"
    ck: FlatCircuit
    expected: Expected

    def matrices(self, g):
        ck = self.ck
        return g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints, *[(m.row_ptr, m.col, m.val) for m in ck.abc])


FIXED = ["edges_good", "empty_a", "empty_c", "wrap_bad", "all_fixed"]


@functools.lru_cache(maxsize=None)
def fixed_case(curve: str, name: str) -> FixedCase:
    """columns: 0 one | 1 x | 2 y | 3 x y | 4 m = p - 1 | 5 w | 6 five.
    good rows: x * y = xy;  m * m = 1 (a = b = p - 1);  and the wrap row -- A, B, C of eight terms (p - 1) * v each, v = p - 1 or w:
    every sum wraps p eight times over, a = b = 8 and c = 8 (p - 1) w = 64 for w = p - 8.
    empty_a: A empty, C = five (c != 0).  empty_c: C empty, a b = x y != 0.  wrap_bad: the wrap row with w = p - 1 (c = 8 != 64)."""
    cp = CP[curve]
    p = cp.r
    rng = pm.SplitMix64(4242 + len(curve))
    x, y = rng.field(p) or 1, rng.field(p) or 1
    w = p - 1 if name in ("wrap_bad", "all_fixed") else p - 8
    z = [1, x, y, x * y % p, p - 1, w, 5]
    good = ([(1, 1)], [(1, 2)], [(1, 3)])
    pm1 = ([(1, 4)], [(1, 4)], [(1, 0)])
    wrap = ([(p - 1, 4)] * 8, [(p - 1, 4)] * 8, [(p - 1, 5)] * 8)
    empty_a = ([], [(1, 2)], [(1, 6)])
    empty_c = ([(1, 1)], [(1, 2)], [])
    rows = {"edges_good": [good, pm1, wrap], "empty_a": [good, empty_a, pm1], "empty_c": [good, pm1, empty_c], "wrap_bad": [good, pm1, wrap],
            "all_fixed": [good, empty_a, empty_c, pm1, wrap]}[name]
    cs = pm.R1CS(2, len(z) - 2, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    return FixedCase(cp, name, cs, circuit_from_pymodel(cp, cs, z), expect(cs, z, p))
