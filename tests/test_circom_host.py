"""CPU tier: the Circom reduction's host side (g16_host_h_query_scalars, g16_h_query_len) against the literal big-int model of
tests/circom_model.py, and the model itself against the CPU oracle's Libsnark map and against itself.

  * h_query_scalars(CIRCOM) == the odd entries of the model's size-2n inverse transform at n = 1, 2, 4, 8, 64 (the library uses
    a closed form with one batch inversion, the model the transform itself);  (LIBSNARK) == zt delta^-1 t^i.
  * for a satisfying assignment A B - C = h_libsnark Z and Z(rho w^k) = rho^n - 1 = -2, so
        h_circom[k] = -2 sum_i h_libsnark[i] rho^i w^(ik)
    with the right-hand side from the oracle's map: ties the model's map to an independent implementation.
  * sum_k h[k] s[k] = delta^-1 (A B - C)(t) for ANY assignment (the even-indexed evaluations of A B - C vanish because c = a b on
    the domain): ties the model's two functions -- and with the first item the library's scalars -- to each other."""
import numpy as np
import pytest

import circom_model as cm
import pymodel as pm
from helpers import circuit_from_pymodel, ints_to_mont, mont_to_ints, ptr64

CURVES = {"bls12_381": pm.BLS12_381, "bn254": pm.BN254}
CID = {"bls12_381": 0, "bn254": 1}
LIBSNARK, CIRCOM = 0, 1
BAD_ARG = 3


@pytest.fixture(scope="module")
def lib():
    import groth16_amd

    return groth16_amd.lib()


def host_scalars(lib, curve, qap, n, t, dinv):
    cp = CURVES[curve]
    out = np.zeros((max(int(lib.c.g16_h_query_len(qap, n)), 1), 4), dtype=np.uint64)
    rc = lib.c.g16_host_h_query_scalars(CID[curve], qap, n, ptr64(ints_to_mont([t], cp.r, 4)), ptr64(ints_to_mont([dinv], cp.r, 4)), ptr64(out))
    return rc, mont_to_ints(out[: int(lib.c.g16_h_query_len(qap, n))], cp.r)


def trapdoor(cp, seed):
    rng = pm.SplitMix64(seed)
    return rng.field(cp.r), rng.field(cp.r)


@pytest.mark.parametrize("curve", sorted(CURVES))
@pytest.mark.parametrize("n", [1, 2, 4, 8, 64])
def test_circom_scalars_equal_literal_inverse_transform(lib, curve, n):
    cp = CURVES[curve]
    t, dinv = trapdoor(cp, 700 + n)
    rc, got = host_scalars(lib, curve, CIRCOM, n, t, dinv)
    assert rc == 0
    want = cm.h_query_scalars(cp, n, t, dinv)
    assert len(got) == n == len(want)
    assert got == want


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_model_transform_sum_and_recursion_agree(curve):
    """the model's plain DFT sums against pymodel's recursion, above the size where it switches"""
    cp = CURVES[curve]
    t, dinv = trapdoor(cp, 711)
    assert 2 * 32 > cm.DFT_SUM_LIMIT
    assert cm.h_query_scalars(cp, 32, t, dinv) == cm.h_query_scalars(cp, 32, t, dinv, force_sum=True)


@pytest.mark.parametrize("curve", sorted(CURVES))
@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_libsnark_scalars(lib, curve, n):
    cp = CURVES[curve]
    p = cp.r
    t, dinv = trapdoor(cp, 720 + n)
    rc, got = host_scalars(lib, curve, LIBSNARK, n, t, dinv)
    assert rc == 0
    zt = (pow(t, n, p) - 1) % p
    assert got == [zt * dinv % p * pow(t, i, p) % p for i in range(n - 1)]


def test_h_query_len(lib):
    for n in (1, 2, 8, 1 << 20):
        assert lib.c.g16_h_query_len(LIBSNARK, n) == n - 1
        assert lib.c.g16_h_query_len(CIRCOM, n) == n
    assert lib.c.g16_h_query_len(2, 8) == 0 and lib.c.g16_h_query_len(-1, 8) == 0
    assert lib.c.g16_h_query_len(CIRCOM, 0) == 0


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_refusals(lib, curve):
    cp = CURVES[curve]
    _, dinv = trapdoor(cp, 730)
    for n in (1, 4, 64):
        _, rho = cm.roots(cp, n)
        for j in (1, 2 * n - 1):
            rc, _ = host_scalars(lib, curve, CIRCOM, n, pow(rho, j, cp.r), dinv)
            assert rc == BAD_ARG, (n, j)
    rc, got = host_scalars(lib, curve, CIRCOM, 4, pow(cm.roots(cp, 4)[1], 2, cp.r), dinv)   # rho^even: defined
    assert rc == 0 and got == cm.h_query_scalars(cp, 4, pow(cm.roots(cp, 4)[1], 2, cp.r), dinv)
    out = np.zeros((8, 4), dtype=np.uint64)
    one = ints_to_mont([5], cp.r, 4)
    for qap in (2, -1, 7):
        assert lib.c.g16_host_h_query_scalars(CID[curve], qap, 8, ptr64(one), ptr64(one), ptr64(out)) == BAD_ARG
    assert lib.c.g16_host_h_query_scalars(CID[curve], CIRCOM, 6, ptr64(one), ptr64(one), ptr64(out)) == BAD_ARG   # no power of two
    assert lib.c.g16_host_h_query_scalars(5, CIRCOM, 8, ptr64(one), ptr64(one), ptr64(out)) == BAD_ARG


def circuits(cp):
    yield "syn3", pm.syn_circuit(cp, 3, 5)
    yield "syn5_dense", pm.syn_circuit(cp, 5, 6, dense=True)
    yield "mimc7", pm.mimc_circuit(cp, 7, 8)     # 14 constraints + 2 inputs: exactly 2^4
    yield "mimc8", pm.mimc_circuit(cp, 8, 9)     # 16 + 2: 2^4 + 2


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_model_map_is_minus_two_times_the_shifted_libsnark_quotient(orc, curve):
    cp = CURVES[curve]
    p = cp.r
    for name, (cs, z) in circuits(cp):
        assert pm.is_satisfied(cs, z, p), name
        h_lib = mont_to_ints(orc.witness_map(circuit_from_pymodel(cp, cs, z)), p)
        n = len(h_lib)
        w, rho = cm.roots(cp, n)
        shifted = [x * pow(rho, i, p) % p for i, x in enumerate(h_lib)]
        want = [(-2 * sum(shifted[i] * pow(w, i * k, p) for i in range(n))) % p for k in range(n)]
        assert cm.witness_map(cp, cs, z) == want, name


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_model_map_and_scalars_give_the_quotient_at_t(curve):
    cp = CURVES[curve]
    p = cp.r
    for name, (cs, z) in circuits(cp):
        for bad in (False, True):
            zz = list(z)
            if bad:
                zz[-1] = (zz[-1] + 1) % p
                assert not pm.is_satisfied(cs, zz, p)
            t, dinv = trapdoor(cp, 740)
            h = cm.witness_map(cp, cs, zz)
            s = cm.h_query_scalars(cp, len(h), t, dinv)
            assert sum(x * y for x, y in zip(h, s)) % p == dinv * cm.abc_at(cp, cs, zz, t) % p, (name, bad)
