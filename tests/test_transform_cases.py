"""Pins the references of the transform edge tests at the edges themselves (CPU only).  The C++ oracle is what the GPU tier
(test_gpu_transform_edges.py) compares with bit for bit; until here it was pinned to the big-int model on random data only.
For every named vector of transform_cases and every (va, vb, vc) triple: oracle == pymodel, plus the closed forms of the
constant and geometric vectors as a third witness that shares no transform code with either."""
import numpy as np
import pytest

import pymodel as pm
import transform_cases as tc
from helpers import ints_to_mont, mont_to_ints

CPS = [pm.BLS12_381, pm.BN254]
SIZES = [1, 2, 3, 5, 8]


def _model(dom, x, inverse, coset, g):
    if coset:
        return dom.coset_ifft(x, g) if inverse else dom.coset_fft(x, g)
    return dom.ifft(x) if inverse else dom.fft(x)


def test_case_generator_is_consistent(orc):
    """the fast conversions equal helpers', the two sources of the random vectors agree, and the named vectors are what their
    names say"""
    for cp in CPS:
        p = cp.r
        xs = [0, 1, p - 1, p - 2, 12345, pm.SplitMix64(4).field(p)]
        assert (tc.to_mont(xs, p) == ints_to_mont(xs, p, 4)).all()
        assert tc.from_mont(tc.to_mont(xs, p), p) == xs == mont_to_ints(tc.to_mont(xs, p), p)
        for n, length in ((2, 1), (8, 8), (32, 31), (256, 255)):
            for name in tc.NAMES:
                ints = tc.vector_ints(cp, name, n, 7, length)
                assert len(ints) == length and all(0 <= v < p for v in ints)
                for o in (None, orc):
                    assert (tc.vector_mont(cp, name, n, 7, length, o) == ints_to_mont(ints, p, 4)).all(), (name, n)
        n = 32
        v = lambda name: tc.vector_ints(cp, name, n, 3)   # noqa: E731
        assert v("zeros") == [0] * n and v("ones") == [1] * n and v("const_pm1") == [p - 1] * n
        for name, at in (("impulse_first", 0), ("impulse_mid", n // 2), ("impulse_last", n - 1)):
            assert v(name) == [p - 1 if i == at else 0 for i in range(n)]
        assert v("alt_pm1_0") == [p - 1, 0] * (n // 2) and v("alt_pm1_1") == [p - 1, 1] * (n // 2)
        assert v("alt_0_pm1") == [0, p - 1] * (n // 2)
        assert v("half_pm1") == [p - 1] * (n // 2) + [0] * (n // 2) and v("half_0_pm1") == [0] * (n // 2) + [p - 1] * (n // 2)
        w = pm.Domain(cp, n).omega_inv
        assert v("geometric_1") == [pow(w, i, p) for i in range(n)]
        assert v("geometric_h") == [pow(w, (n // 2 + 1) * i, p) for i in range(n)]
        plain, edged = v("rand"), v("rand_edges")
        changed = [i for i in range(n) if plain[i] != edged[i]]
        assert len(changed) == n // 8 and all(edged[i] in (0, 1, p - 1) for i in range(n) if i in changed)
        assert sorted(i // 8 for i in changed) == list(range(n // 8))
    need = {("const_pm1",) * 3, ("const_pm1", "const_pm1", "zeros"), ("zeros", "rand", "rand"), ("alt_pm1_1", "alt_pm1_0", "const_pm1"),
            ("impulse_first", "impulse_mid", "impulse_last"), ("rand_edges",) * 3, ("rand", "rand", "product"), ("rand",) * 3}
    have = {tuple(name for name, _ in t) for t in tc.TRIPLES.values()}
    assert need <= have and any(all(nm.startswith("geometric") for nm in t) for t in have)
    assert set(tc.TRIPLES_AT_19) <= set(tc.TRIPLES)


@pytest.mark.parametrize("cp", CPS, ids=lambda c: c.name)
@pytest.mark.parametrize("log_n", SIZES)
def test_oracle_ntt_matches_model_on_named_vectors(orc, cp, log_n):
    n, p, g = 1 << log_n, cp.r, cp.fr_generator
    dom = pm.Domain(cp, n)
    for name in tc.NAMES:
        x = tc.vector_ints(cp, name, n, 60 + log_n)
        xa = tc.vector_mont(cp, name, n, 60 + log_n)
        for inverse, coset in tc.MODES:
            got = orc.ntt(cp.name, xa, inverse, coset)
            assert tc.from_mont(got, p) == _model(dom, x, inverse, coset, g), (name, inverse, coset)
        # closed forms (no transform code): a constant c -> n c at index 0; w^(-j i) -> n at index j
        fwd = tc.from_mont(orc.ntt(cp.name, xa, False, False), p)
        if name in ("zeros", "ones", "const_pm1"):
            assert fwd == [n * x[0] % p] + [0] * (n - 1), name
        if name.startswith("geometric_"):
            j = tc.geometric_index(name, n)
            assert fwd == [n % p if i == j else 0 for i in range(n)], name


@pytest.mark.parametrize("cp", CPS, ids=lambda c: c.name)
@pytest.mark.parametrize("k", SIZES)
def test_oracle_witness_map_matches_model_on_free_vectors(orc, cp, k):
    """the library and the models refuse nothing for an unsatisfied system: h = (a b - c) / Z on the coset either way"""
    p = cp.r
    for tname in tc.TRIPLES:
        va, vb, vc = tc.triple_mont(cp, k, tname)
        for coeff in (1, p - 1):
            ck = tc.free_vector_circuit(cp.name, k, va, vb, vc, coeff)
            assert ck.domain_size == 1 << k and ck.num_vars == len(ck.z)
            cs, z = tc.r1cs_of(ck)
            h_py, (a_py, b_py, c_py) = pm.witness_map_from_matrices(cp, cs, z, want_abc=True)
            # the circuit hands the map the three vectors themselves (times coeff), a closed by the instance's 1
            ints = [tc.from_mont(v, p) for v in (va, vb, vc)]
            assert a_py == [coeff * x % p for x in ints[0]] + [1]
            assert b_py == [coeff * x % p for x in ints[1]] + [0] and c_py == [coeff * x % p for x in ints[2]] + [0]
            h_or, abc_or = orc.witness_map(ck, want_abc=True)
            assert [tc.from_mont(m, p) for m in abc_or] == [a_py, b_py, c_py], tname
            assert tc.from_mont(h_or, p) == h_py, (tname, coeff)
            if tname == "satisfied" and coeff == 1:
                assert pm.is_satisfied(cs, z, p) and h_py[-1] == 0
            if tname == "pm1_all" and coeff == 1 and k > 1:
                assert not pm.is_satisfied(cs, z, p)


def test_triples_at_two_to_the_nineteen_are_cheap_to_build(orc):
    """the k = 19 circuit of the GPU tier: built from numpy arrays, no Python loop over rows"""
    cp = pm.BN254
    va, vb, vc = tc.triple_mont(cp, 19, "pm1_all", orc)
    ck = tc.free_vector_circuit(cp.name, 19, va, vb, vc)
    assert ck.num_constraints == (1 << 19) - 1 and ck.domain_size == 1 << 19
    assert ck.abc[2].col[0] == 1 + 2 * ck.num_constraints and int(ck.abc[2].col[-1]) == ck.num_vars - 1
    assert (ck.z[1:] == tc.to_mont([cp.r - 1], cp.r)[0]).all() and (ck.z[0] == tc.to_mont([1], cp.r)[0]).all()
