"""CPU tier, no library: the premises of lagrange_cases.py against the big-int model.  Every edge input meets, in some stage of the
transform, the collision it is named after -- an identity operand, equal operands (the sum is a doubling, the difference the
identity), opposite operands, a doubling of a point with y = 0 -- and the points of order 3 r tell the library's twiddle rule
(min(w, r - w), then a negation) from a plain multiplication by w."""
import pytest

import lagrange_cases as lc
import pymodel as pm
import table_cases as tc

CURVES = ["bls12_381", "bn254"]
LOG_N = lc.LOG_NS[0]

# label prefix -> what must be seen: (operation, kind) in any stage, or (stage, operation, kind)
NEEDS = {
    "identities": [(0, "sum", "ZERO"), (0, "diff", "ZERO")],
    "identities between points": [(0, "sum", "ZERO"), ("sum", "TAKE_Q"), ("diff", "TAKE_Q")],
    "points between identities": [(0, "sum", "ZERO"), ("sum", "TAKE_P"), ("diff", "TAKE_P"), ("sum", "ADD")],
    "constant": [(0, "sum", "DBL"), (0, "diff", "ZERO"), (1, "sum", "DBL"), (1, "sum", "ZERO")],
    "P, -P in turn": [(0, "sum", "DBL"), (0, "diff", "ZERO"), ("sum", "ZERO"), ("diff", "DBL")],
    "multiples of P": [("sum", "ADD"), ("diff", "ADD")],
    "order two, constant": [(0, "sum", "ZERO"), (0, "diff", "ZERO")],
    "order two between identities": [("sum", "TAKE_P"), ("sum", "TAKE_Q"), ("sum", "ZERO")],
    "multiples of a point of order three": [("sum", "DBL"), ("sum", "ZERO"), ("diff", "DBL"), ("diff", "ZERO")],
    "multiples of a point of order four": [("sum", "DBL"), ("sum", "ZERO"), ("diff", "ZERO")],
    "small order": [("sum", "ZERO"), ("diff", "ZERO")],   # (order two: nothing else; the union over the class is held below)
    "k G + T, order 3 r on the curve": [("sum", "ADD"), ("diff", "ADD")],
}


def _needs(label):
    return NEEDS["small order"] if label.startswith("small order") else NEEDS[label]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("curve", CURVES)
def test_every_edge_input_meets_its_collision(curve, g2):
    small, anywhere = set(), set()
    for label, pts in lc.edge_inputs(curve, g2, LOG_N):
        seen = set()
        for inverse in (False, True):
            lc.model_transform(curve, g2, pts, inverse, seen)
        for need in _needs(label):
            if len(need) == 3:
                assert need in seen, (label, need, sorted(seen))
            else:
                assert any(x[1:] == need for x in seen), (label, need, sorted(seen))
        if "order" in label:
            small |= {x[1:] for x in seen if x[0] > 0}
            anywhere |= {x[1:] for x in seen}
    # among the small-order inputs equal and opposite operands arise AFTER stage 0, where the operands are the transform's own values
    assert {("sum", "DBL"), ("sum", "ZERO"), ("diff", "ZERO")} <= small, sorted(small)
    assert ("diff", "DBL") in anywhere


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("curve", CURVES)
def test_the_two_reduced_sizes_hold_the_same_classes(curve, g2):
    assert [label for label, _ in lc.edge_inputs(curve, g2, lc.LOG_NS[1])] == lc.edge_ids(curve, g2)


def test_the_twiddle_rule_matters_outside_the_subgroup():
    """on k G + T the library's rule and a plain multiplication by w differ by multiples of r T = +-T; on subgroup points they agree"""
    curve, g2 = "bls12_381", False
    inputs = dict(lc.edge_inputs(curve, g2, LOG_N))
    pts = inputs["k G + T, order 3 r on the curve"]
    m = tc.model(curve, g2)
    r = pm.CURVES[curve].r
    assert r % 3 != 0 and m.add(m.dbl((0, 2)), (0, 2)) is None
    assert lc.model_transform(curve, g2, pts, True) != lc.model_transform(curve, g2, pts, True, plain=True)
    sub = inputs["multiples of P"]
    assert lc.model_transform(curve, g2, sub, True) == lc.model_transform(curve, g2, sub, True, plain=True)


@pytest.mark.parametrize("curve", CURVES)
def test_model_transform_is_the_dft_sum(curve):
    """the stages of the model against the plain sum over points, on subgroup points where both are defined"""
    import srs_cases as sc

    cp = pm.CURVES[curve]
    G1 = pm.groups(cp)[0]
    pts = dict(lc.edge_inputs(curve, False, LOG_N))["multiples of P"]
    dom = pm.Domain(cp, len(pts))
    assert lc.model_transform(curve, False, pts, False) == sc.model_group_dft(G1, pts, dom.omega, cp.r)
    assert lc.model_transform(curve, False, pts, True) == sc.model_group_dft(G1, pts, dom.omega_inv, cp.r, dom.n_inv)
