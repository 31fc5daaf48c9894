"""GPU tier: the device standard-form lab (g16_dev_std_op) against the models on the shared cases of tests/std_cases.py -- both
curves, every kind (Fr, Fq, Fq2, G1, G2), every form.  This is the device's own Montgomery product (Fp::mul_cios32, which no CPU test
reaches through operator*) and the group law above it, as the row walks, the quotient and power kernels, the fixed-base and srs_*
kernels and the verifiers' XYZZ records run them, on operands no whole operation on honest inputs supplies: products whose value
before reduce_once is in [p, 2 p), sums equal to p, rows with m = 0, XYZZ pairs equal under different scales, records with zz = 0
and stale coordinates.  Field results are compared bit for bit with the model; group results as affine points, with zz^3 = zzz^2
checked on every raw record.  The device's output must also equal the host twin's word for word: for mul / sqr / from_canonical the
twin's 32-bit-body forms (mul32 / sqr32 / from_canonical32), for everything else the same form (every output is canonical, so the
host's 64-bit product cannot show).

Every form is launched with n = 1, 63, 64, 65 tuples (first and last lane, a partial and a full wavefront, a second workgroup) and
once with every case cycled to 2049 tuples or more; mul_bits, whose lanes run for milliseconds, is cycled to 129.  The output buffer
is pre-filled with a sentinel.  Cases, expected values and the host twin's outputs are made once per (curve, kind, form)."""
import ctypes as C
import functools

import numpy as np
import pytest

import std_cases as sc

pytestmark = pytest.mark.gpu

BIG, BIG_LONG = 2049, 129   # 32 full wavefronts and one lane; two and one lane for the scalar multiples
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lab():
    import groth16_amd

    lib = groth16_amd.lib()
    ctxs = {}
    for curve, cid in sc.fc.CURVE_ID.items():
        ctx = C.c_void_p()
        lib.check(lib.c.g16_ctx_create(cid, 0, C.byref(ctx)))
        ctxs[curve] = ctx
    yield lib, ctxs
    for ctx in ctxs.values():
        lib.c.g16_ctx_destroy(ctx)


@functools.lru_cache(maxsize=None)
def host_outputs(curve, kind, form):
    """the host twin on the form's cases, through the device's product where the form has such a twin"""
    _, ops = sc.operands(curve, kind, form)
    return sc.run_host(curve, kind, sc.TWIN32.get(form, form) if kind in ("fr", "fq") else form, ops)


def run_batch(lib, ctx, curve, kind, form, n):
    fid, nin, nout = sc.slots(kind, form)
    N = sc.words_per_slot(curve, kind)
    cs, ops = sc.operands(curve, kind, form, n)
    base = len(sc.cases(curve, kind, form))
    assert ops.shape == (n, nin, N), (form, ops.shape)
    out = np.full((n, nout, N), 0xDEADBEEF, dtype=np.uint32)
    lib.check(lib.c.g16_dev_std_op(ctx, sc.KIND[kind], fid, ops.ctypes.data_as(U32P), n, out.ctypes.data_as(U32P)))
    for i, (c, o) in enumerate(zip(cs, out)):
        try:
            c.check(o)
        except AssertionError as e:
            raise AssertionError("n = %d, tuple %d (lane %d of workgroup %d): %s" % (n, i, i % 64, i // 64, e)) from None
    host = host_outputs(curve, kind, form)
    same = (out == host[np.arange(n) % base]).reshape(n, -1).all(axis=1)
    assert same.all(), "n = %d: tuple %d (%s) differs from the host twin" % (n, int(np.argmin(same)), cs[int(np.argmin(same))].what)


@pytest.mark.parametrize("curve,kind,form", sc.PARAMS, ids=["%s-%s-%s" % p for p in sc.PARAMS])
def test_gpu_std_lab(lab, curve, kind, form):
    lib, ctxs = lab
    for n in (1, 63, 64, 65):
        run_batch(lib, ctxs[curve], curve, kind, form, n)
    run_batch(lib, ctxs[curve], curve, kind, form, max(len(sc.cases(curve, kind, form)), BIG_LONG if form == "mul_bits" else BIG))


def test_gpu_std_lab_refusals(lab):
    lib, ctxs = lab
    buf = np.zeros(20 * 12, dtype=np.uint32)
    out = np.zeros(8 * 12, dtype=np.uint32)
    p, o = buf.ctypes.data_as(U32P), out.ctypes.data_as(U32P)
    f, ctx = lib.c.g16_dev_std_op, ctxs["bn254"]
    for kind, form in ((0, -1), (0, 10), (0, 19), (1, 13), (2, 7), (2, 14), (3, 7), (4, 14), (-1, 0), (5, 0)):
        assert f(ctx, kind, form, p, 1, o) != 0, (kind, form)
    assert f(ctx, 0, 0, p, 0, o) != 0 and f(ctx, 0, 0, p, (1 << 22) + 1, o) != 0
    assert f(ctx, 0, 0, None, 1, o) != 0 and f(ctx, 0, 0, p, 1, None) != 0
    assert f(None, 0, 0, p, 1, o) != 0
