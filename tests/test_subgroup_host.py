"""CPU tier: the endomorphism membership tests of subgroup.hpp through g16_host_check_subgroups, against multiplication by r in the
big-int model on the shared case list (identity, members, random curve points, a point of every small prime order dividing the
cofactor, member + torsion, off-curve), and against the host deserialiser's Validate::Yes."""
import numpy as np
import pytest

import groth16_amd as g
from groth16_amd.serialize import deserialize_points, serialize_points
from subgroup_cases import EXPECTED_PRIMES, NAMES, case_arrays, cases

GROUPS = [False, True]


@pytest.mark.parametrize("g2", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_the_model(name, g2):
    labels, pts, want = case_arrays(name, g2)
    got = g.check_subgroups_host(name, pts, g2)
    assert got.dtype == np.uint8
    assert {lb: int(f) for lb, f in zip(labels, got)} == {lb: int(f) for lb, f in zip(labels, want)}


@pytest.mark.parametrize("g2", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_torsion_list(name, g2):
    """non-empty for the three groups with a cofactor, empty for BN254 G1 (h = 1)"""
    _, torsion = cases(name, g2)
    assert sorted(torsion) == EXPECTED_PRIMES[(name, int(g2))]
    assert bool(torsion) == (not (name == "bn254" and not g2))


@pytest.mark.parametrize("g2", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_agrees_with_validating_deserialiser(name, g2):
    """every on-curve point, after a serialise round trip: g16_deserialize_points(validate=2) accepts it iff the flag is 1"""
    labels, pts, want = case_arrays(name, g2)
    got = g.check_subgroups_host(name, pts, g2)
    for label, p, f in zip(labels, pts, got):
        if f == 2:
            continue
        data = serialize_points(name, p, g2, compressed=False)
        assert (deserialize_points(name, data, 1, g2, compressed=False, validate=1)[0] == p).all(), label
        try:
            deserialize_points(name, data, 1, g2, compressed=False, validate=2)
            accepted = True
        except g.G16Error as e:
            assert e.status == 9, label
            accepted = False
        assert accepted == (f == 1), label


@pytest.mark.parametrize("g2", GROUPS)
@pytest.mark.parametrize("name", NAMES)
def test_flags_keep_their_order(name, g2):
    _, pts, want = case_arrays(name, g2)
    perm = np.random.default_rng(5).permutation(len(want))
    assert (g.check_subgroups_host(name, pts[perm], g2) == want[perm]).all()


@pytest.mark.parametrize("name", NAMES)
def test_empty(name):
    for g2 in GROUPS:
        out = g.check_subgroups_host(name, np.zeros((0, 4), dtype=np.uint64).reshape(0), g2)
        assert out.shape == (0,) and out.dtype == np.uint8
    lb = g.lib()
    assert lb.c.g16_host_check_subgroups(0, 0, None, 0, None) == 0
    assert lb.c.g16_host_check_subgroups(7, 0, None, 0, None) == 3     # unknown curve
    assert lb.c.g16_host_check_subgroups(0, 2, None, 0, None) == 3     # g2 is 0 or 1
