"""CPU tier: g16_host_decode_points -- the templates the key loader's kernels run, compiled for the host -- against the host reader
point by point (status 1 iff g16_deserialize_points accepts that one point, and then the same limbs) and against the big-int
model's labels (the non-1 statuses say WHY, which the reader does not), for every case of key_bytes_cases, both encodings and the
three validation levels."""
import numpy as np
import pytest

import key_bytes_cases as kc
from subgroup_cases import NAMES

import groth16_amd as g
from groth16_amd.serialize import deserialize_points, serialize_points

GROUPS = [(name, g2, compressed) for name in NAMES for g2 in (False, True) for compressed in (True, False)]
IDS = [f"{n}-{'g2' if g2 else 'g1'}-{'compressed' if c else 'uncompressed'}" for n, g2, c in GROUPS]


@pytest.mark.parametrize("name,g2,compressed", GROUPS, ids=IDS)
@pytest.mark.parametrize("validate", kc.VALIDATE)
def test_host_decode_matches_reader_and_model(name, g2, compressed, validate):
    labels, encs, status, points = kc.cases(name, g2, compressed)
    got_pts, got_st = g.decode_points_host(name, kc.blob(encs), g2, compressed, validate)
    assert got_st.tolist() == status[validate].tolist(), [(l, int(a), int(b)) for l, a, b in zip(labels, got_st, status[validate]) if a != b]
    assert got_pts.tobytes() == points[validate].tobytes()
    for label, enc, st, pt in zip(labels, encs, got_st, got_pts):
        try:
            want = deserialize_points(name, enc, 1, g2, compressed=compressed, validate=validate)
        except g.InvalidData:
            want = None
        assert (want is not None) == (st == 1), (label, int(st))
        if want is not None:
            assert want[0].tobytes() == pt.tobytes(), label
        else:
            assert not pt.any(), label   # the identity is stored whenever the status is not 1


@pytest.mark.parametrize("name,g2,compressed", GROUPS, ids=IDS)
def test_case_lists_cover_what_they_claim(name, g2, compressed):
    labels, encs, status, points = kc.cases(name, g2, compressed)
    assert set(status[0].tolist()) == {0, 1}          # no on-curve test without validation
    if not compressed:
        assert 2 in status[1] and 2 in status[2]      # only the uncompressed form can name a point off the curve
        assert (status[1][status[0] == 0] == 0).all()
        # the writer's own encodings are among the valid ones: the generator as the library serialises it
        assert serialize_points(name, points[0][labels.index("member0")], g2, compressed=False) == encs[labels.index("member0")]
        assert ("wrong_sign_flag" in labels) == (name == "bn254")
        assert ("compressed_bit_set" in labels and "sign_bit_set" in labels) == (name == "bls12_381")
    else:
        assert 2 not in status[1] and 2 not in status[2]
    if name == "bn254" and not g2:
        assert 3 not in status[2]                     # cofactor 1: there is no point to make this case from
    else:
        assert 3 in status[2]
    assert 3 not in status[1]


def test_empty_input_and_bad_arguments():
    lb = g.lib()
    assert lb.c.g16_host_decode_points(0, 0, 1, 2, None, 0, None, None) == 0
    out = np.zeros(24, dtype=np.uint64)
    st = np.zeros(1, dtype=np.uint8)
    for curve, g2, compressed, validate in ((2, 0, 1, 2), (0, 2, 1, 2), (0, 0, 2, 2), (0, 0, 1, 3), (0, 0, 1, -1)):
        assert lb.c.g16_host_decode_points(curve, g2, compressed, validate, bytes(192), 1, g.binding.ptr64(out), st.ctypes.data) == 3
    assert lb.c.g16_host_decode_points(0, 0, 1, 2, None, 1, g.binding.ptr64(out), st.ctypes.data) == 3
    assert lb.c.g16_decode_points(None, 0, 1, 2, bytes(48), 1, g.binding.ptr64(out), st.ctypes.data) == 3
