"""CPU tier: the host twin of the standard-form lab (g16_host_std_op: field.hpp and curve.hpp compiled for the host, one operation per
tuple on the ABI's words) against the models of tests/std_cases.py -- every form, kind and curve, every case -- and its refusals.
The product forms run twice: mul / sqr / from_canonical through operator* (the host's 64-bit body, what the host glue runs per proof)
and mul32 / sqr32 / from_canonical32 through Fp::mul_cios32 by name (the device's body); both are compared with the model and with
each other.  The forms g16_host_field_op / g16_host_group_op also have must agree with them."""
import ctypes as C

import numpy as np
import pytest

import std_cases as sc

import groth16_amd

U32P = C.POINTER(C.c_uint32)
U64P = C.POINTER(C.c_uint64)


@pytest.mark.parametrize("curve,kind,form", sc.PARAMS, ids=["%s-%s-%s" % p for p in sc.PARAMS])
def test_host_std_lab(curve, kind, form):
    cs, ops = sc.operands(curve, kind, form)
    out = sc.run_host(curve, kind, form, ops)
    sc.check_all(cs, out)
    twin = {v: k for k, v in sc.TWIN32.items()}
    if kind in ("fr", "fq") and form in twin:        # the device's body against the host's, word for word
        assert (sc.run_host(curve, kind, twin[form], ops) == out).all()


FIELD_OPS = {"add": 0, "sub": 1, "mul": 2, "inverse": 3, "to_canonical": 4, "from_canonical": 5}
FIELD_PARAMS = [(curve, kind, form) for curve in sc.CURVES for kind in ("fr", "fq") for form in FIELD_OPS]


@pytest.mark.parametrize("curve,kind,form", FIELD_PARAMS, ids=["%s-%s-%s" % p for p in FIELD_PARAMS])
def test_host_field_op_agrees(curve, kind, form):
    lib = groth16_amd.lib()
    cs, ops = sc.operands(curve, kind, form)
    out = sc.run_host(curve, kind, form, ops)
    N = sc.words_per_slot(curve, kind)
    got = np.zeros(N // 2, dtype=np.uint64)
    for i in range(0, len(cs), 3 if form == "inverse" else 1):
        a = np.ascontiguousarray(ops[i, 0]).view(np.uint64)
        b = np.ascontiguousarray(ops[i, 1]).view(np.uint64) if ops.shape[1] == 2 else None
        rc = lib.c.g16_host_field_op(sc.fc.CURVE_ID[curve], sc.KIND[kind], FIELD_OPS[form], a.ctypes.data_as(U64P),
                                     b.ctypes.data_as(U64P) if b is not None else None, got.ctypes.data_as(U64P))
        assert rc == 0 and (got.view(np.uint32) == out[i, 0]).all(), cs[i].what


@pytest.mark.parametrize("curve", sc.CURVES)
@pytest.mark.parametrize("kind", ("g1", "g2"))
def test_host_group_op_agrees(curve, kind):
    """g16_host_group_op's p + q (op 0: from_affine, add_affine, to_affine) and k p (op 1: from_affine, mul_bits over 256 bits,
    to_affine) against the lab's add_affine / mul_bits followed by its to_affine"""
    lib = groth16_amd.lib()
    g2 = int(kind == "g2")
    N = sc.words_per_slot(curve, kind)
    c = 1 + g2
    cs, ops = sc.operands(curve, kind, "add_affine")
    aff = sc.run_host(curve, kind, "to_affine", sc.run_host(curve, kind, "add_affine", ops))
    got = np.zeros(2 * c * N // 2, dtype=np.uint64)
    for i in range(len(cs)):
        p, q = (np.ascontiguousarray(ops[i, j * 2 * c:(j + 1) * 2 * c]).reshape(-1).view(np.uint64) for j in (0, 1))
        assert lib.c.g16_host_group_op(sc.fc.CURVE_ID[curve], g2, 0, p.ctypes.data_as(U64P), q.ctypes.data_as(U64P), got.ctypes.data_as(U64P)) == 0
        assert (got.view(np.uint32) == aff[i].reshape(-1)).all(), cs[i].what
    # k p: the lab's cases whose record is an affine point under scale 1 and whose bit count is 256
    cs, ops = sc.operands(curve, kind, "mul_bits")
    aff = sc.run_host(curve, kind, "to_affine", sc.run_host(curve, kind, "mul_bits", ops))
    one = np.array(sc.std(curve, "fq").words(sc.std(curve, "fq").Rp), dtype=np.uint32)
    n = 0
    for i in range(len(cs)):
        zz, zzz = ops[i, 2 * c:3 * c], ops[i, 3 * c:4 * c]
        if int(ops[i, 4 * c + 1, 0]) != 256 or not ((zz[0] == one).all() and (zzz[0] == one).all() and not zz[1:].any() and not zzz[1:].any()):
            continue
        p = np.ascontiguousarray(ops[i, :2 * c]).reshape(-1).view(np.uint64)
        k = np.ascontiguousarray(ops[i, 4 * c, :8]).view(np.uint64)
        assert lib.c.g16_host_group_op(sc.fc.CURVE_ID[curve], g2, 1, p.ctypes.data_as(U64P), k.ctypes.data_as(U64P), got.ctypes.data_as(U64P)) == 0
        assert (got.view(np.uint32) == aff[i].reshape(-1)).all(), cs[i].what
        n += 1
    assert n >= 8


def test_host_std_lab_refusals():
    lib = groth16_amd.lib()
    buf = np.zeros(20 * 12, dtype=np.uint32)
    out = np.zeros(8 * 12, dtype=np.uint32)
    p, o = buf.ctypes.data_as(U32P), out.ctypes.data_as(U32P)
    f = lib.c.g16_host_std_op
    for curve in (0, 1):
        for kind in sc.KIND:
            for form in sc.forms(kind):
                assert f(curve, sc.KIND[kind], sc.slots(kind, form)[0], p, 1, o) == 0, (curve, kind, form)
    for kind, bad in ((0, (-1, 10, 11, 12, 13, 16, 17, 19, 1000)), (1, (-1, 10, 13, 16, 17, 19)), (2, (-1, 7, 8, 9, 14, 15, 18)), (3, (-1, 7, 14)), (4, (-1, 7, 14))):
        for form in bad:
            assert f(0, kind, form, p, 1, o) != 0, (kind, form)
    assert f(0, -1, 0, p, 1, o) != 0 and f(0, 5, 0, p, 1, o) != 0
    assert f(0, 0, 0, p, 0, o) != 0 and f(0, 0, 0, p, (1 << 22) + 1, o) != 0
    assert f(0, 0, 0, None, 1, o) != 0 and f(0, 0, 0, p, 1, None) != 0
    assert f(2, 0, 0, p, 1, o) != 0 and f(-1, 0, 0, p, 1, o) != 0


def test_form_table_is_the_headers():
    assert sorted(v[0] for v in sc.FP_FORMS.values()) == list(range(10)) + [14, 15, 18]
    assert sorted(v[0] for v in sc.FP2_FORMS.values()) == list(range(7)) == sorted(v[0] for v in sc.GROUP_FORMS.values())
    assert sc.slots("g2", "mul_bits") == (5, 10, 8) and sc.slots("g1", "add") == (1, 8, 4) and sc.slots("g2", "to_affine") == (6, 8, 4)
