"""The R1CS satisfaction check on the MI355X (run with -m gpu): g16_circuit_check against its host twin on every case of
check_cases.py -- both curves, both reductions (Circom with C attached), the assignment in host memory and resident on the device --
and g16_prove_checked: the same proof bit for bit as g16_prove for a satisfying assignment, Unsatisfiable and no proof otherwise.
The host twin itself is tied to the big-int model in test_r1cs_check_host.py (CPU tier)."""
import ctypes as C
import random

import numpy as np
import pytest

import check_cases as cc
import pymodel as pm

pytestmark = pytest.mark.gpu

BAD_ARG = 3
QAPS = ["libsnark", "circom"]


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module", params=[(c, q) for c in cc.CURVES for q in QAPS], ids=lambda p: "%s-%s" % p)
def env(request, g):
    curve, qap = request.param
    prover = g.Groth16(curve, 0, qap=g.CircomReduction if qap == "circom" else g.LibsnarkReduction)
    yield curve, qap, prover
    prover.close()


def device_copy(z):
    import torch

    return torch.from_numpy(np.ascontiguousarray(z).view(np.int64)).cuda()


def assert_same(got, want, where):
    """field for field"""
    assert got.n_unsatisfied == want.n_unsatisfied, where
    assert got.first_row == want.first_row, where
    for k in "abc":
        assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), (where, k)


@pytest.mark.parametrize("ni", cc.NIS)
@pytest.mark.parametrize("nc", cc.NCS)
def test_check_equals_host_twin(env, g, nc, ni):
    curve, qap, prover = env
    bs = cc.base(curve, nc, ni)
    mats = bs.matrices(g)
    for name, rows in cc.bad_sets(nc):
        case = cc.case(curve, nc, ni, name)
        want = g.host_check_assignment(curve, mats, case.z)
        assert want.n_unsatisfied == len(rows)
        assert_same(prover.check_assignment(mats, case.z), want, (name, "host assignment"))
        z_dev = device_copy(case.z)
        assert_same(prover.check_assignment(mats, None, z_dev_ptr=z_dev.data_ptr()), want, (name, "device assignment"))
        assert prover.is_satisfied(mats, case.z) == (not rows)
        assert prover.which_is_unsatisfied(mats, case.z) == (rows[0] if rows else None)
    prover.evict()


@pytest.mark.parametrize("name", cc.FIXED)
def test_fixed_rows_equal_host_twin(env, g, name):
    curve, qap, prover = env
    fc = cc.fixed_case(curve, name)
    mats = fc.matrices(g)
    want = g.host_check_assignment(curve, mats, fc.ck.z)
    assert want.n_unsatisfied == fc.expected.n_unsatisfied and want.first_row == fc.expected.first_row
    assert_same(prover.check_assignment(mats, fc.ck.z), want, "host assignment")
    z_dev = device_copy(fc.ck.z)
    assert_same(prover.check_assignment(mats, None, z_dev_ptr=z_dev.data_ptr()), want, "device assignment")
    prover.evict()


@pytest.mark.parametrize("curve", cc.CURVES)
def test_circom_needs_c_attached(g, curve):
    """a Circom circuit holds A and B only: the check refuses it until g16_circuit_attach_c has brought C, and the map, which never
    reads C, gives the same h before and after"""
    from groth16_amd.binding import CheckResultC

    case = cc.case(curve, 257, 2, "block_edge")
    mats = case.base.matrices(g)
    z = case.z
    with g.Groth16(curve, 0, qap=g.CircomReduction) as prover:
        lb, ctx = prover._ctx.lib, prover._ctx.handle
        dck = prover._ck(mats)
        res = CheckResultC()
        h_before = prover.witness_map_from_matrices(mats, 2, 257, z)
        rc = lb.c.g16_circuit_check(ctx, dck.handle, z.ctypes.data, z.shape[0], 0, C.byref(res))
        assert rc == BAD_ARG
        with pytest.raises(g.G16Error) as e:
            lb.check(rc)
        assert e.value.status == BAD_ARG and "g16_circuit_attach_c" in str(e.value)
        dck.attach_c(mats)
        assert lb.c.g16_circuit_check(ctx, dck.handle, z.ctypes.data, z.shape[0], 0, C.byref(res)) == 0
        assert (res.n_unsatisfied, res.first_row) == (2, 255)
        dck._has_c = False
        dck.attach_c(mats)      # a second call replaces nothing
        assert lb.c.g16_circuit_check(ctx, dck.handle, z.ctypes.data, z.shape[0], 0, C.byref(res)) == 0
        assert (res.n_unsatisfied, res.first_row) == (2, 255)
        assert lb.c.g16_circuit_check(ctx, dck.handle, z.ctypes.data, z.shape[0] - 1, 0, C.byref(res)) == 2     # G16_ERR_BAD_LENGTH
        h_after = prover.witness_map_from_matrices(mats, 2, 257, z)
        assert h_before.tobytes() == h_after.tobytes() and h_before.any()


class Chain:
    """u_(i+2) = u_i u_(i+1), nc constraints; the last value is the public input"""

    def __init__(self, p, nc, seed):
        rng = pm.SplitMix64(seed)
        self.u = [rng.field(p), rng.field(p)]
        for i in range(nc):
            self.u.append(self.u[i] * self.u[i + 1] % p)

    def generate_constraints(self, cs):
        from groth16_amd import lc

        nc = len(self.u) - 2
        x = cs.new_input_variable(lambda: self.u[-1])
        v = [cs.new_witness_variable(lambda j=j: self.u[j]) for j in range(nc + 1)] + [x]
        for i in range(nc):
            cs.enforce_constraint(lc() + v[i], lc() + v[i + 1], lc() + v[i + 2])


def chain_inputs(g, curve, nc):
    from groth16_amd.r1cs import synthesize

    circuit = Chain(cc.CP[curve].r, nc, 5 + nc)
    cs = synthesize(curve, circuit, setup_mode=False)
    assert cs.is_satisfied() and cs.num_constraints == nc
    return circuit, cs.to_matrices(), cs.full_assignment()


def fixed_r_s(curve, seed):
    from groth16_amd.groth16 import _rand_fr

    rng = random.Random(seed)
    return _rand_fr(curve, rng), _rand_fr(curve, rng)


@pytest.mark.parametrize("nc", [1 << 4, (1 << 7) + 1, 1 << 10], ids=["2^4", "2^7+1", "2^10"])
def test_checked_proof_equals_unchecked(env, g, nc):
    curve, qap, prover = env
    circuit, mats, z = chain_inputs(g, curve, nc)
    pk, vk = prover.setup(circuit, random.Random(nc))      # generate_parameters with this prover's reduction
    r, s = fixed_r_s(curve, 100 + nc)
    want = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, 2, nc, z)      # check=False: the existing path, the yardstick
    got = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, 2, nc, z, check=True)
    assert got.flat().tobytes() == want.flat().tobytes()
    pvk = prover.prepare_verifying_key(vk)
    assert prover.verify_proof(pvk, got, [z[1]])

    # one witness entry bumped: no proof, the first failing row as the host twin names it
    bad = z.copy()
    k = 2 + nc // 2
    bad[k] = z[k - 1]
    assert bad[k].tobytes() != z[k].tobytes()
    twin = g.host_check_assignment(curve, mats, bad)
    assert twin.n_unsatisfied > 0
    with pytest.raises(g.Unsatisfiable) as e:
        prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, 2, nc, bad, check=True)
    assert e.value.status == 12 and e.value.row == twin.first_row and e.value.n_unsatisfied == twin.n_unsatisfied
    assert e.value.a.tobytes() == twin.a.tobytes() and e.value.b.tobytes() == twin.b.tobytes() and e.value.c.tobytes() == twin.c.tobytes()
    # unchecked, the bad witness still "proves" (the reference's release behaviour): a well-formed proof the verifier rejects
    garbage = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, 2, nc, bad)
    assert not prover.verify_proof(pvk, garbage, [bad[1]])
    # the context is left usable: the good witness through the same context, unchecked and checked
    again = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, 2, nc, z)
    assert again.flat().tobytes() == want.flat().tobytes()
    again = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, 2, nc, z, check=True)
    assert again.flat().tobytes() == want.flat().tobytes()
    pvk.close()
    prover.evict()


def test_checked_proof_through_the_circuit_level_calls(env, g):
    """check= on create_proof_with_reduction / create_proof_no_zk / prove, and on PipelinedProver.submit"""
    curve, qap, prover = env
    nc = 40
    circuit, mats, z = chain_inputs(g, curve, nc)
    pk, vk = prover.setup(circuit, random.Random(3))
    r, s = fixed_r_s(curve, 9)
    want = prover.create_proof_with_reduction(circuit, pk, r, s)
    assert prover.create_proof_with_reduction(circuit, pk, r, s, check=True).flat().tobytes() == want.flat().tobytes()
    assert prover.create_proof_no_zk(circuit, pk, check=True).flat().tobytes() == prover.create_proof_no_zk(circuit, pk).flat().tobytes()
    pvk = prover.prepare_verifying_key(vk)
    assert prover.verify_proof(pvk, prover.prove(pk, circuit, random.Random(4), check=True), [z[1]])
    broken = Chain(cc.CP[curve].r, nc, 5 + nc)
    broken.u[7] = (broken.u[7] + 1) % cc.CP[curve].r
    with pytest.raises(g.Unsatisfiable) as e:
        prover.create_proof_with_reduction(broken, pk, r, s, check=True)
    assert e.value.row == 5       # u_7 is first read as the product of row 5
    pvk.close()
    prover.evict()
    with g.PipelinedProver(curve, 0, qap=prover.qap) as pp:
        futs = [pp.submit(pk, r, s, mats, 2, nc, z, check=bool(i & 1)) for i in range(4)]
        assert all(f.result().flat().tobytes() == want.flat().tobytes() for f in futs)
        bad = z.copy()
        bad[9] = z[8]
        with pytest.raises(g.Unsatisfiable):
            pp.submit(pk, r, s, mats, 2, nc, bad, check=True).result()
        assert pp.submit(pk, r, s, mats, 2, nc, z).result().flat().tobytes() == want.flat().tobytes()


@pytest.mark.parametrize("curve", cc.CURVES)
def test_multi_device_context_checks_on_its_first_device(g, curve):
    """two contexts over the one visible GPU: the check runs on the first, the answer is the single-device one; a checked proof
    is the unchecked proof of the same context"""
    nc = (1 << 7) + 1
    case = cc.case(curve, 1000, 2, "random_1pct")
    mats = case.base.matrices(g)
    want = g.host_check_assignment(curve, mats, case.z)
    assert want.n_unsatisfied == 10
    circuit, cmats, z = chain_inputs(g, curve, nc)
    r, s = fixed_r_s(curve, 77)
    with g.Groth16(curve, [0, 0]) as multi:
        assert_same(multi.check_assignment(mats, case.z), want, "host assignment")
        z_dev = device_copy(case.z)
        assert_same(multi.check_assignment(mats, None, z_dev_ptr=z_dev.data_ptr()), want, "device assignment")
        assert multi.is_satisfied(mats, case.base.ck.z)
        with g.Groth16(curve, 0) as single:
            pk, _ = single.setup(circuit, random.Random(12))
        plain = multi.create_proof_with_reduction_and_matrices(pk, r, s, cmats, 2, nc, z)
        checked = multi.create_proof_with_reduction_and_matrices(pk, r, s, cmats, 2, nc, z, check=True)
        assert checked.flat().tobytes() == plain.flat().tobytes()
        bad = z.copy()
        bad[5] = z[4]
        with pytest.raises(g.Unsatisfiable) as e:
            multi.create_proof_with_reduction_and_matrices(pk, r, s, cmats, 2, nc, bad, check=True)
        assert e.value.row == g.host_check_assignment(curve, cmats, bad).first_row
        assert multi.create_proof_with_reduction_and_matrices(pk, r, s, cmats, 2, nc, z).flat().tobytes() == plain.flat().tobytes()
