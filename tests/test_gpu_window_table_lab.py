"""GPU tier: the key loader's window-table builder in place -- build_window_tables with its chunk loop, the parking buffer it
allocates and its launch shape, hence build_window_tables_kernel, window_table_task, jac30_double, TableDeviceIO and one
division-step inversion per point -- through g16_dev_window_table_lab, on the points of tests/table_cases.py, against the big-int
affine doubling: row j of point i must be the canonical packed words of 2^(c j) P_i (x R', y R' with R' = 2^(30 NL)), an identity row
all zero, bit for bit.

Whole MSMs and proofs only ever hand the builder points of the prime-order subgroup: no Z ever has a zero component, no point reaches
the identity.  Here (x, 0) leaves through the task's `live` exit after one doubling, (0, y) has order 3, the G2 points with a zero
component in y or x make the two lanes of a pair disagree (in Z's zero test and in load()'s identity test), and a G2 point of order 4
reaches the identity through a Y that is a computed multiple of p.  Shapes: (c, W) = (1, 2), (3, 1), (5, 4), (8, 32), (16, 16),
(20, 13) with n = 1, 63, 64, 65 and one n whose tasks span three workgroups, every point class on the first and on the last task of
a wave (two layouts for G2, which has more classes than the launch has full waves).

The second chunk of the builder's loop (n > 2^18 points) stays with the full-size tests (tests/test_gpu_fullsize.py): a lab call
of that size would cost more than this whole module."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc
import table_cases as tc

pytestmark = pytest.mark.gpu

G16_OK, G16_ERR_BAD_ARG, G16_ERR_INTERNAL = 0, 3, 7
CONFIGS = [(curve, g2) for curve in fc.CURVE_ID for g2 in (0, 1)]
CONFIG_IDS = ["%s-%s" % (curve, "g2" if g2 else "g1") for curve, g2 in CONFIGS]


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


def points_array(m, pts):
    return np.array([tc.abi_words(m, P) for P in pts], dtype=np.uint64)


def check_table(lab, curve, g2, c, W, n, layout):
    from groth16_amd import binding

    lib, ctxs = lab
    m = tc.model(curve, g2)
    pts, edges = tc.table_points(curve, g2, n, layout)
    names = {P: name for name, cl in tc.point_classes(curve, g2) for P in cl}
    status, got = binding.window_table_lab(lib, ctxs[curve], g2, points_array(m, pts), c, W)
    lib.check(status)
    want = np.array(tc.expected_table(curve, g2, pts, c, W), dtype=np.uint64)
    assert got.shape == want.shape == (W, n, len(tc.abi_words(m, None)))
    bad = np.argwhere((got != want).any(axis=2))
    if len(bad):
        j, i = (int(x) for x in bad[0])
        T = tc.tasks_per_wave(g2)
        raise AssertionError("%s %s, c = %d, W = %d, n = %d, layout %d: %d of %d rows differ; first: row %d of point %d (%s%s; task %d of wave %d): "
                             "got %s, 2^%d P = %s" % (curve, "G2" if g2 else "G1", c, W, n, layout, len(bad), W * n, j, i, names[pts[i]],
                                                      ", a wave-edge task" if i in edges else "", i % T, i // T, tc.decode_row(m, got[j][i]), c * j,
                                                      m.chain(pts[i], c * j)))
    return edges


@pytest.mark.parametrize("shape", tc.SHAPES, ids=["c%d-W%d" % s for s in tc.SHAPES])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_window_table_rows(lab, cfg, shape):
    curve, g2 = cfg
    c, W = shape
    for k, n in enumerate(tc.SIZES):
        check_table(lab, curve, g2, c, W, n, k)   # (another rotation of the pool per size: every class meets task 0)
    on_edges = set()
    T, big = tc.tasks_per_wave(g2), tc.big_n(g2)
    assert 2 * tc.TABLE_THREADS < big * (2 if g2 else 1) <= 3 * tc.TABLE_THREADS   # three workgroups
    for layout in range(tc.layouts(curve, g2)):
        edges = check_table(lab, curve, g2, c, W, big, layout)
        for name in set(edges.values()):
            assert {t % T for t, v in edges.items() if v == name} == {0, T - 1}
            on_edges.add(name)
    assert on_edges == {name for name, _ in tc.point_classes(curve, g2)}


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_window_table_lab_refusals(lab, cfg):
    from groth16_amd import binding

    lib, ctxs = lab
    curve, g2 = cfg
    m = tc.model(curve, g2)
    pts, _ = tc.table_points(curve, g2, 3)
    arr = points_array(m, pts)
    fill = 0xDEADBEEFDEADBEEF
    status, out = binding.window_table_lab(lib, ctxs[curve], g2, arr, 5, 33)
    assert status == G16_ERR_INTERNAL and (out == fill).all()      # the builder's own limit; nothing was launched
    status, out = binding.window_table_lab(lib, ctxs[curve], g2, arr[:0], 5, 4)
    assert status == G16_OK and out.shape[1] == 0
    buf = np.full(8 * arr.shape[1], fill, dtype=np.uint64)          # n = 0 with real buffers behind the pointers: nothing is written
    u64p = C.POINTER(C.c_uint64)
    assert lib.c.g16_dev_window_table_lab(ctxs[curve], g2, arr.ctypes.data_as(u64p), 0, 5, 4, buf.ctypes.data_as(u64p)) == G16_OK
    assert (buf == fill).all()
    for c, W in ((0, 4), (33, 4), (5, 0), (5, 65)):
        assert binding.window_table_lab(lib, ctxs[curve], g2, arr, c, W)[0] == G16_ERR_BAD_ARG, (c, W)
    assert lib.c.g16_dev_window_table_lab(ctxs[curve], g2, arr.ctypes.data_as(u64p), (1 << 18) + 4097, 5, 4, buf.ctypes.data_as(u64p)) == G16_ERR_BAD_ARG
    assert lib.c.g16_dev_window_table_lab(None, g2, arr.ctypes.data_as(u64p), 3, 5, 4, buf.ctypes.data_as(u64p)) == G16_ERR_BAD_ARG
    assert lib.c.g16_dev_window_table_lab(ctxs[curve], g2, None, 3, 5, 4, buf.ctypes.data_as(u64p)) == G16_ERR_BAD_ARG
    status, got = binding.window_table_lab(lib, ctxs[curve], g2, arr, 5, 4)   # the context still works after the refusals
    assert status == G16_OK and (got == np.array(tc.expected_table(curve, g2, pts, 5, 4), dtype=np.uint64)).all()
