"""GPU tier: the device tower lab (g16_dev_pairing_op) against the exact model on the shared cases of tests/tower_cases.py, both
curves, every form: Q30 and the T2 / T6 / T12 operations, the Frobenius maps, equal / store_gt / load_gt, ell, the projective
doubling and addition steps, frob_twist, cyc_pow / cyc_pow_bits / exp_by_x, final_exp and the on-curve tests.  On the device these
routines are out of line and pass their Fq12 values through scratch call frames, which the host twin (test_tower_host.py) cannot
show.  Every result component must be a normalised limb vector below 2 p with the model's residue; flags and stored words are
compared exactly.

Every form is launched with n = 1, 63, 64, 65 tuples (first and last lane, a partial and a full wavefront, a second workgroup) and
once with every case cycled to 2049 tuples or more; final_exp and cyc_pow_bits, whose lanes run for milliseconds, are cycled to 129
(two wavefronts and one lane cover the indexing).  The output buffer is pre-filled with a sentinel.  The cases and their expected
values are made once per (curve, form) and shared by the launch sizes (tower_cases.cases is cached).

The kernels are milliseconds; the cost is the Python model.  Making the cases of one form with their expected values, measured on
the build machine (one core, CPU seconds, BLS12-381 / BN254): the Q30 and T2 forms 0.00 - 0.01; the T6 forms 0.01 - 0.04; t12_mul 0.08 /
0.07, the other T12 forms, equal, store_gt, load_store_gt and ell 0.01 - 0.04; frob 0.12 / 0.04; frob_twist 0.03 / 0.12; dbl_step
0.19 / 0.11; add_step 0.10 / 0.12; cyc_pow 0.33 / 0.24; exp_by_x 0.32 / 0.30; cyc_pow_bits 1.02 / 0.84; final_exp 2.57 / 0.95 (four
F.pow by (q^12 - 1) / r and two model Miller loops per curve); t12_cyc_sqr 1.32 / 0.68, nearly all of it the one-time tables that the
first cyclotomic form pays (w^(q^j), three easy-part powers); g1_on_curve 1.27 / 0.12 and g2_on_curve 0.72 / 0.35, nearly all of it
the torsion points of subgroup_cases.  12.7 s for all 94 (curve, form) pairs; checking a 2049-tuple launch adds 0.02 - 0.5 s.  On the
GPU machine the 95 tests of this file and the 40 of test_gpu_verify.py took 24 s together, the slowest of this file 1.1 s.  No form
needed its random tuples reduced."""
import ctypes as C

import numpy as np
import pytest

import tower_cases as tc

pytestmark = pytest.mark.gpu

PARAMS = [(curve, form) for curve in tc.CURVES for form in tc.FORMS]
BIG, BIG_LONG = 2049, 129   # 32 full wavefronts and one lane; two and one lane for the long chains
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lab():
    import groth16_amd

    lib = groth16_amd.lib()
    ctxs = {}
    for curve, cid in tc.fc.CURVE_ID.items():
        ctx = C.c_void_p()
        lib.check(lib.c.g16_ctx_create(cid, 0, C.byref(ctx)))
        ctxs[curve] = ctx
    yield lib, ctxs
    for ctx in ctxs.values():
        lib.c.g16_ctx_destroy(ctx)


def run_batch(lib, ctx, curve, form, cases):
    fid, nin, nout = tc.FORMS[form]
    NL = tc.ctx(curve).NL
    ops = np.ascontiguousarray(np.array([c.slots for c in cases], dtype=np.uint32))
    assert ops.shape == (len(cases), nin, NL), (form, ops.shape)
    out = np.full((len(cases), nout, NL), 0xDEADBEEF, dtype=np.uint32)
    lib.check(lib.c.g16_dev_pairing_op(ctx, fid, ops.ctypes.data_as(U32P), len(cases), out.ctypes.data_as(U32P)))
    for i, (c, o) in enumerate(zip(cases, out)):
        try:
            c.check(o)
        except AssertionError as e:
            raise AssertionError("n = %d, tuple %d (lane %d of workgroup %d): %s" % (len(cases), i, i % 64, i // 64, e)) from None


@pytest.mark.parametrize("curve,form", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_gpu_tower_lab(lab, curve, form):
    lib, ctxs = lab
    cases = tc.cases(curve, form)
    assert len(cases) >= 65
    for n in (1, 63, 64, 65):
        run_batch(lib, ctxs[curve], curve, form, cases[:n])
    n_big = max(len(cases), BIG_LONG if form in tc.LONG_FORMS else BIG)
    run_batch(lib, ctxs[curve], curve, form, [cases[i % len(cases)] for i in range(n_big)])


def test_gpu_tower_lab_refusals(lab):
    lib, ctxs = lab
    buf = np.zeros(24 * 13, dtype=np.uint32)
    out = np.zeros(13 * 13, dtype=np.uint32)
    p, o = buf.ctypes.data_as(U32P), out.ctypes.data_as(U32P)
    f, ctx = lib.c.g16_dev_pairing_op, ctxs["bn254"]
    for form in (-1, 21, 36, 46, 64):
        assert f(ctx, form, p, 1, o) != 0, form
    assert f(ctx, 0, p, 0, o) != 0 and f(ctx, 0, p, (1 << 22) + 1, o) != 0
    assert f(ctx, 0, None, 1, o) != 0 and f(ctx, 0, p, 1, None) != 0
    assert f(None, 0, p, 1, o) != 0
