"""CPU tier: g16_host_circuit_check -- the satisfaction check's row walk compiled for the host, the comparator of the GPU tier --
against oracle/pymodel.py (is_satisfied / evaluate_constraint) on every case of check_cases.py, and the ABI around the check."""
import ctypes as C

import numpy as np
import pytest

import check_cases as cc
import pymodel as pm
from helpers import circuit_from_pymodel, ints_to_mont, mont_to_ints

import groth16_amd as g
from groth16_amd import binding
from groth16_amd.binding import CURVE_ID, CheckResultC, CsrViewC, ptr32, ptr64

BAD_LENGTH, BAD_ARG, UNSATISFIED = 2, 3, 12


def assert_matches_model(res, ex, p):
    assert res.satisfied == (ex.n_unsatisfied == 0)
    assert res.n_unsatisfied == ex.n_unsatisfied
    assert res.first_row == ex.first_row
    if ex.abc is None:
        assert not (res.a.any() or res.b.any() or res.c.any())
    else:
        assert tuple(mont_to_ints(np.stack([res.a, res.b, res.c]), p)) == ex.abc


@pytest.mark.parametrize("curve,nc,ni", [(c, nc, ni) for c in cc.CURVES for nc in cc.NCS for ni in cc.NIS])
def test_host_check_equals_model(curve, nc, ni):
    bs = cc.base(curve, nc, ni)
    mats = bs.matrices(g)
    for name, _ in cc.bad_sets(nc):
        case = cc.case(curve, nc, ni, name)
        assert_matches_model(g.host_check_assignment(curve, mats, case.z), case.expected, bs.cp.r)


@pytest.mark.parametrize("curve", cc.CURVES)
@pytest.mark.parametrize("name", cc.FIXED)
def test_host_check_fixed_rows(curve, name):
    fc = cc.fixed_case(curve, name)
    want_bad = {"edges_good": 0, "empty_a": 1, "empty_c": 1, "wrap_bad": 1, "all_fixed": 3}[name]
    assert fc.expected.n_unsatisfied == want_bad     # the model agrees with what the rows were written to be
    assert_matches_model(g.host_check_assignment(curve, fc.matrices(g), fc.ck.z), fc.expected, fc.cp.r)


@pytest.mark.parametrize("curve", cc.CURVES)
def test_host_check_mimc(curve):
    cp = cc.CP[curve]
    cs, z = pm.mimc_circuit(cp, 40, 11)
    ck = circuit_from_pymodel(cp, cs, z)
    mats = g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints, *[(m.row_ptr, m.col, m.val) for m in ck.abc])
    assert pm.is_satisfied(cs, z, cp.r)
    assert_matches_model(g.host_check_assignment(curve, mats, ck.z), cc.expect(cs, z, cp.r), cp.r)
    for k in (2, 3, 17, len(z) - 1):       # one witness entry bumped
        z2 = list(z)
        z2[k] = (z2[k] + 1) % cp.r
        ex = cc.expect(cs, z2, cp.r)
        assert ex.n_unsatisfied > 0 and not pm.is_satisfied(cs, z2, cp.r)
        assert_matches_model(g.host_check_assignment(curve, mats, ints_to_mont(z2, cp.r, 4)), ex, cp.r)


def test_constraint_system_which_is_unsatisfied():
    """the thin synthesis layer's own loop, next to is_satisfied"""
    p = cc.CP["bn254"].r

    class Two:
        def __init__(self, off):
            self.off = off

        def generate_constraints(self, cs):
            x = cs.new_input_variable(lambda: 6)
            a = cs.new_witness_variable(lambda: 2)
            b = cs.new_witness_variable(lambda: 3)
            c = cs.new_witness_variable(lambda: 36 + self.off)
            cs.enforce_constraint(g.lc() + a, g.lc() + b, g.lc() + x)
            cs.enforce_constraint(g.lc() + x, g.lc() + x, g.lc() + c)

    from groth16_amd.r1cs import synthesize
    good, bad = synthesize("bn254", Two(0), False), synthesize("bn254", Two(1), False)
    assert good.is_satisfied() and good.which_is_unsatisfied() is None
    assert not bad.is_satisfied() and bad.which_is_unsatisfied() == 1
    res = g.host_check_assignment("bn254", bad.to_matrices(), bad.full_assignment())
    assert (res.n_unsatisfied, res.first_row) == (1, 1)
    assert mont_to_ints(np.stack([res.a, res.b, res.c]), p) == [6, 6, 37]


def test_bad_length_and_null_arguments():
    lb = g.lib()
    fc = cc.fixed_case("bls12_381", "edges_good")
    ck = fc.ck
    views = (CsrViewC * 3)(*[CsrViewC(ptr64(m.row_ptr), ptr32(m.col), ptr64(m.val)) for m in ck.abc])
    res = CheckResultC()
    call = lb.c.g16_host_circuit_check
    assert call(0, views, ck.num_constraints, ck.z.ctypes.data, ck.num_vars, C.byref(res)) == 0 and res.n_unsatisfied == 0
    assert res.first_row == 2 ** 64 - 1
    # an assignment shorter than the columns the rows read
    assert call(0, views, ck.num_constraints, ck.z.ctypes.data, 4, C.byref(res)) == BAD_LENGTH
    assert call(0, None, ck.num_constraints, ck.z.ctypes.data, ck.num_vars, C.byref(res)) == BAD_ARG
    assert call(0, views, ck.num_constraints, None, ck.num_vars, C.byref(res)) == BAD_ARG
    assert call(0, views, ck.num_constraints, ck.z.ctypes.data, ck.num_vars, None) == BAD_ARG
    assert call(7, views, ck.num_constraints, ck.z.ctypes.data, ck.num_vars, C.byref(res)) == BAD_ARG
    null_rows = (CsrViewC * 3)(views[0], views[1], CsrViewC(None, None, None))
    assert call(0, null_rows, ck.num_constraints, ck.z.ctypes.data, ck.num_vars, C.byref(res)) == BAD_ARG
    bad_rp = ck.abc[2].row_ptr.copy()
    bad_rp[1] = bad_rp[-1] + 1     # row_ptr[1] > row_ptr[2]: decreasing
    dec = (CsrViewC * 3)(views[0], views[1], CsrViewC(ptr64(bad_rp), ptr32(ck.abc[2].col), ptr64(ck.abc[2].val)))
    assert call(0, dec, ck.num_constraints, ck.z.ctypes.data, ck.num_vars, C.byref(res)) == BAD_LENGTH
    # no constraints: nothing is read, nothing fails
    assert call(1, views, 0, ck.z.ctypes.data, ck.num_vars, C.byref(res)) == 0
    assert (res.n_unsatisfied, res.first_row) == (0, 2 ** 64 - 1)
    # the entry points that need a context refuse a NULL one before anything else
    assert lb.c.g16_circuit_check(None, None, None, 0, 0, C.byref(res)) == BAD_ARG
    assert lb.c.g16_circuit_attach_c(None, None, None) == BAD_ARG
    assert lb.c.g16_prove_checked(None, None, None, None, 0, 0, None, None, None, None) == BAD_ARG


def test_status_text_and_struct_size():
    lb = g.lib()
    assert lb.c.g16_strerror(UNSATISFIED).decode().startswith("unsatisfied")
    assert lb.c.g16_struct_size(7) == C.sizeof(CheckResultC) == 112
    assert lb.c.g16_abi_version() == 2
    with pytest.raises(g.Unsatisfiable) as e:
        lb.check(UNSATISFIED)
    assert e.value.status == UNSATISFIED and isinstance(e.value, g.SynthesisError) and e.value.row is None
    res = CheckResultC(3, 5)
    with pytest.raises(g.Unsatisfiable) as e:
        lb.check(UNSATISFIED, res)
    assert (e.value.row, e.value.n_unsatisfied) == (5, 3) and e.value.a.shape == (4,)
    assert {"g16_circuit_attach_c", "g16_circuit_check", "g16_prove_checked", "g16_host_circuit_check"} <= set(binding.EXPORTS)
