"""CPU tier: the host twin of the tower lab (g16_host_pairing_op: the pairing.hpp templates compiled for the host, one operation per
tuple on raw limbs) against the exact model of tests/tower_cases.py -- every form, both curves, every case -- its refusals, and the
model helpers that tower_cases adds to pymodel / pairing_model (from_ark, the cheap Frobenius and inverse) pinned against F.pow."""
import ctypes as C
import random

import numpy as np
import pytest

import pairing_model as pmod
import tower_cases as tc

import groth16_amd

PARAMS = [(curve, form) for curve in tc.CURVES for form in tc.FORMS]
U32P = C.POINTER(C.c_uint32)


def run_host(curve, form, cases):
    lib = groth16_amd.lib()
    fid, nin, nout = tc.FORMS[form]
    NL = tc.ctx(curve).NL
    ops = np.ascontiguousarray(np.array([c.slots for c in cases], dtype=np.uint32))
    assert ops.shape == (len(cases), nin, NL), (form, ops.shape)
    out = np.full((len(cases), nout, NL), 0xDEADBEEF, dtype=np.uint32)
    rc = lib.c.g16_host_pairing_op(tc.fc.CURVE_ID[curve], fid, ops.ctypes.data_as(U32P), len(cases), out.ctypes.data_as(U32P))
    assert rc == 0, (curve, form, rc)
    return out


@pytest.mark.parametrize("curve,form", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_host_tower_lab(curve, form):
    cases = tc.cases(curve, form)
    assert len(cases) >= 65
    out = run_host(curve, form, cases)
    for i, (c, o) in enumerate(zip(cases, out)):
        try:
            c.check(o)
        except AssertionError as e:
            raise AssertionError("tuple %d: %s" % (i, e)) from None


def test_operand_dump_for_the_replay_program(tmp_path):
    """the file tests/tower_lab_replay.cpp reads: one record per (curve, form), operands and this build's outputs"""
    path = tmp_path / "tower_lab.bin"
    n = tc.dump_operands(str(path), run_host)
    assert n == len(PARAMS)
    words = np.fromfile(str(path), dtype="<u4")
    pos = 0
    for curve, form in PARAMS:
        cid, fid, cnt, nin, nout, NL = (int(x) for x in words[pos:pos + 6])
        assert (cid, fid, nin, nout, NL) == (tc.fc.CURVE_ID[curve], *tc.FORMS[form], tc.ctx(curve).NL) and cnt == len(tc.cases(curve, form))
        pos += 6 + cnt * (nin + nout) * NL
    assert pos == len(words)


def test_host_tower_lab_refusals():
    lib = groth16_amd.lib()
    buf = np.zeros(24 * 13, dtype=np.uint32)
    out = np.zeros(13 * 13, dtype=np.uint32)
    p, o = buf.ctypes.data_as(U32P), out.ctypes.data_as(U32P)
    f = lib.c.g16_host_pairing_op
    assert f(0, 0, p, 1, o) == 0
    for form in (-1, 21, 29, 36, 46, 49, 64, 1000):   # the gaps between the levels and what lies past the last form
        assert f(0, form, p, 1, o) != 0, form
    assert f(0, 0, p, 0, o) != 0 and f(0, 0, p, (1 << 22) + 1, o) != 0
    assert f(0, 0, None, 1, o) != 0 and f(0, 0, p, 1, None) != 0
    assert f(2, 0, p, 1, o) != 0 and f(-1, 0, p, 1, o) != 0


def test_form_table_is_the_headers():
    ids = sorted(v[0] for v in tc.FORMS.values())
    assert ids == list(range(0, 10)) + list(range(10, 21)) + list(range(30, 36)) + list(range(40, 46)) + list(range(50, 64))


@pytest.mark.parametrize("curve", tc.CURVES)
def test_model_helpers(curve):
    cx = tc.ctx(curve)
    F, p = cx.F, cx.p
    rng = random.Random("tower/helpers/%s" % curve)
    els = [[rng.randrange(p) for _ in range(12)] for _ in range(2)]
    for a in els:
        assert tc.from_ark(curve, pmod.to_ark(curve, a)) == a
        ark = [rng.randrange(p) for _ in range(12)]
        assert pmod.to_ark(curve, tc.from_ark(curve, ark)) == ark
        for j in (1, 2, 3):
            assert tc.frob(curve, a, j) == F.pow(a, p ** j), j
        assert tc.conj(curve, a) == tc.frob(curve, tc.frob(curve, a, 3), 3)
        assert F.mul(a, tc.inv(curve, a)) == F.one
    # arkworks' order: the unit, and v = w^2 in slot c0.c1
    assert tc.from_ark(curve, [1] + [0] * 11) == F.one
    assert tc.from_ark(curve, [0, 0, 1] + [0] * 9) == [0, 0, 1] + [0] * 9
    # u = w^6 - s
    assert tc.from_ark(curve, [0, 1] + [0] * 10) == F.from_fq2((0, 1))
