"""GPU tier: the device field lab (g16_dev_fp30_op) against the big-int model on the shared edge cases (tests/fp30_cases.py), both
curves, every form.  On the device the product forms run the generated assembly blocks themselves and the lane-pair forms run with
their DPP moves live -- the CPU tier (test_fips_asm_emulated.py) can only emulate the former and call the latter's per-lane halves.

Product forms, the carry / subtraction helpers and the canonicalisers are compared limb for limb, the zero tests as flags, the Fq2
forms as residues with the promised bound per component, the accumulator forms (a lazy XYZZ accumulator through a chain of mixed
additions: G1, G2 in one lane and G2 on the lane pair; and the bucket pass's own parked, sign-tracking accumulator in its LDS layout
through signed additions and the flush's gather(): G1 and G2 on the lane pair) as canonical affine points against pymodel's group law.  Every form is
launched with n = 1, 63, 64, 65 tuples (first and last lane, a partial and a full wavefront, a second workgroup) and once with
every case, cycled to more than two thousand tuples."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc

pytestmark = pytest.mark.gpu

FIELDS = fc.fields()
PARAMS = [(f, form) for f in FIELDS for form in fc.lab_forms(f)]
BIG = 2049   # 32 full wavefronts and one lane


@pytest.fixture(scope="module")
def lab():
    import groth16_amd

    lib = groth16_amd.lib()
    ctxs = {}
    for curve, cid in fc.CURVE_ID.items():
        ctx = C.c_void_p()
        lib.check(lib.c.g16_ctx_create(cid, 0, C.byref(ctx)))
        ctxs[curve] = ctx
    yield lib, ctxs
    for ctx in ctxs.values():
        lib.c.g16_ctx_destroy(ctx)


def run_batch(lib, ctx, f, form, cases):
    fid, nin, nout = fc.LAB[form]
    ops = np.ascontiguousarray(np.array([c.slots for c in cases], dtype=np.uint32))
    assert ops.shape == (len(cases), nin, f.NL), (form, ops.shape)
    out = np.full((len(cases), nout, f.NL), 0xDEADBEEF, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    lib.check(lib.c.g16_dev_fp30_op(ctx, fc.FIELD_ID[f.which], fid, ops.ctypes.data_as(u32p), len(cases), out.ctypes.data_as(u32p)))
    for i, (c, o) in enumerate(zip(cases, out)):
        try:
            c.check(o)
        except AssertionError as e:
            lanes = (2 * i, 2 * i + 1) if form.startswith("pair_") or form.endswith("_pair") else (i,)
            raise AssertionError("%s %s, n = %d, tuple %d (lanes %s): %s" % (f.name, form, len(cases), i, lanes, e)) from None


@pytest.mark.parametrize("f,form", PARAMS, ids=["%s-%s" % (f.name, form) for f, form in PARAMS])
def test_gpu_field_lab(lab, f, form):
    lib, ctxs = lab
    cases = fc.lab_cases(f, form)
    assert len(cases) >= 65
    for n in (1, 63, 64, 65):
        run_batch(lib, ctxs[f.curve], f, form, cases[:n])
    n_big = max(len(cases), BIG)
    run_batch(lib, ctxs[f.curve], f, form, [cases[i % len(cases)] for i in range(n_big)])


def test_gpu_field_lab_rejects_what_it_does_not_have(lab):
    lib, ctxs = lab
    buf = np.zeros(16 * 13, dtype=np.uint32)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    ctx = ctxs["bn254"]
    assert lib.c.g16_dev_fp30_op(ctx, 0, 4, p, 1, p) != 0 and lib.c.g16_dev_fp30_op(ctx, 1, 27, p, 1, p) != 0
    assert lib.c.g16_dev_fp30_op(ctx, 1, 12, p, 1, p) != 0 and lib.c.g16_dev_fp30_op(ctx, 1, 0, p, 0, p) != 0
    assert lib.c.g16_dev_fp30_op(None, 1, 0, p, 1, p) != 0
