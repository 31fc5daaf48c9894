"""CPU tier: the decompression templates (decompress.hpp) through g16_host_decompress_points against the case list of
decompress_cases.py -- status and bytes, both curves, both groups -- the round trip through serialize_points, and the argument
checks of the entry point."""
import ctypes as C

import numpy as np
import pytest

import pymodel as pm
from decompress_cases import NAMES, blob, cases, enc_size

import groth16_amd as g
from groth16_amd.binding import CURVE_ID, ptr64
from groth16_amd.serialize import serialize_points


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_case_list(name, g2):
    labels, encs, status, pts = cases(name, g2)
    got_pts, got_status = g.decompress_points_host(name, blob(encs), g2)
    for label, s, w in zip(labels, got_status, status):
        assert s == w, label
    for label, p, w in zip(labels, got_pts, pts):
        assert p.tobytes() == w.tobytes(), label
    assert 0 in status and 1 in status
    # one point at a time: no state is carried from one point to the next
    for label, enc, s, w in zip(labels, encs, status, pts):
        p1, s1 = g.decompress_points_host(name, enc, g2)
        assert s1[0] == s and p1[0].tobytes() == w.tobytes(), label


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_round_trip(name, g2):
    labels, encs, status, _ = cases(name, g2)
    valid = [i for i in range(len(labels)) if status[i]]
    data = blob(encs, valid)
    pts, st = g.decompress_points_host(name, np.frombuffer(data, dtype=np.uint8), g2)
    assert (st == 1).all()
    assert serialize_points(name, pts, g2) == data


@pytest.mark.parametrize("name", NAMES)
def test_arguments(name):
    lb = g.lib()
    fn = lb.c.g16_host_decompress_points
    curve = CURVE_ID[name]
    L = pm.CURVES[name].fq_limbs64
    _, encs, _, _ = cases(name, False)
    buf = np.frombuffer(blob(encs[:2]), dtype=np.uint8).copy()
    out, st = np.zeros(4 * L, dtype=np.uint64), np.zeros(2, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    bad = 3   # G16_ERR_BAD_ARG
    assert fn(7, 0, p(buf), 2, ptr64(out), p(st)) == bad        # no such curve
    assert fn(curve, 2, p(buf), 2, ptr64(out), p(st)) == bad    # g2 is 0 or 1
    assert fn(curve, 0, None, 2, ptr64(out), p(st)) == bad
    assert fn(curve, 0, p(buf), 2, None, p(st)) == bad
    assert fn(curve, 0, p(buf), 2, ptr64(out), None) == bad
    assert fn(curve, 0, p(buf), 2, ptr64(out), p(st)) == 0
    # n = 0 needs no buffers
    assert fn(curve, 0, None, 0, None, None) == 0 and fn(curve, 1, None, 0, None, None) == 0
    pts, status = g.decompress_points_host(name, b"", True)
    assert pts.shape == (0, 4 * L) and status.shape == (0,)
    for g2 in (False, True):
        with pytest.raises(ValueError):
            g.decompress_points_host(name, bytes(enc_size(name, g2) + 1), g2)
    with pytest.raises(ValueError):
        g.decompress_points_host(name, np.zeros(enc_size(name, False), dtype=np.uint16), False)
