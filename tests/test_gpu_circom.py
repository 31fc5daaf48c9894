"""The Circom R1CS -> QAP reduction on the MI355X (run with -m gpu): the map's kernels bit for bit against the literal big-int
model of circom_model.py, the map at size against the Libsnark map of the same circuit, and Groth16(qap=CircomReduction) end to
end through setup, prove, sharded prove and the verifiers.

What ties the model itself down is in test_circom_host.py (CPU tier).  The identity used at size is the same one: for a
satisfying assignment A B - C = h_libsnark Z and Z = -2 on the odd coset, so h_circom = fft(-2 rho^i h_libsnark[i]).

Key / circuit mix-up, as the length rules give it (prover.hpp: h_start + h_count <= n): a Circom circuit proved with the Libsnark
key of the same circuit passes the check -- that key's h_query is one base SHORT, n - 1 <= n -- and the proof is rejected by the
verifier; test_libsnark_key_with_circom_circuit asserts exactly that.

Window tables: g16_pk_get_info reports window_bits_h > 0 for every key the default settings load (merged windows at every size),
so the smallest end-to-end size already runs the 2^k-base h-query through the merged-plan sort;
test_window_table_key_two_classes adds a two-class merged plan (c = 17) over 2^16 bases."""
import ctypes as C

import numpy as np
import pytest

import circom_model as cm
import pymodel as pm
import transform_cases as tc
from helpers import Csr, FlatCircuit, ints_to_mont, mont_to_ints

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
CP = {"bls12_381": pm.BLS12_381, "bn254": pm.BN254}
BAD_ARG = 3


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module", params=CURVES)
def env(request, g):
    circom = g.Groth16(request.param, 0, qap=g.CircomReduction)
    libsnark = g.Groth16(request.param, 0)
    yield request.param, circom, libsnark
    circom.close()
    libsnark.close()


def mats_of(g, ck):
    return g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints, *[(m.row_ptr, m.col, m.val) for m in ck.abc])


def gpu_map(prover, g, ck):
    h = prover.witness_map_from_matrices(mats_of(g, ck), ck.num_inputs, ck.num_constraints, ck.z)
    prover.evict()
    return h


# ---------------------------------------------------------------------------------------------------------------------------
# map against the model
# ---------------------------------------------------------------------------------------------------------------------------
def random_circuit(cp, nc, ni, seed, satisfied):
    """nc constraints over ni instance and 2 nc + 3 witness variables: A and B rows of 0 - 3 terms with coefficients 1, p - 1 and
    random ones (row i % 5 == 3 of A and row i % 7 == 2 of B are empty); C row i is the single witness variable holding a_i b_i
    (satisfied) or that value plus one in the last row (not satisfied)"""
    p = cp.r
    rng = pm.SplitMix64(seed)
    nfree = nc + 3
    z = [1] + [rng.field(p) for _ in range(ni - 1 + nfree)]

    def row(i, skip):
        if skip:
            return []
        out = []
        for _ in range(1 + rng.next() % 3):
            cf = (1, p - 1, rng.field(p), rng.field(p))[rng.next() % 4]
            out.append((cf, rng.next() % len(z)))
        return out

    A = [row(i, i % 5 == 3) for i in range(nc)]
    B = [row(i, i % 7 == 2) for i in range(nc)]
    Cm = []
    for i in range(nc):
        v = pm.evaluate_constraint(A[i], z, p) * pm.evaluate_constraint(B[i], z, p) % p
        if not satisfied and i == nc - 1:
            v = (v + 1) % p
        Cm.append([(1, len(z))])
        z.append(v)
    cs = pm.R1CS(ni, len(z) - ni, A, B, Cm)
    assert nc == 0 or pm.is_satisfied(cs, z, p) == satisfied
    return cs, z


SHAPES = [(k, 0) for k in range(11)] + [(k, 1) for k in range(10)]   # nc + ni = 2^k, and 2^k + 1 (domain 2^(k + 1))


@pytest.mark.parametrize("k,extra", SHAPES, ids=["2^%d+%d" % s for s in SHAPES])
def test_map_equals_model(env, g, k, extra):
    from helpers import circuit_from_pymodel

    curve, circom, _ = env
    cp = CP[curve]
    total = (1 << k) + extra
    for ni, satisfied in ((1, True), (2, False)):
        if total < ni:
            continue
        cs, z = random_circuit(cp, total - ni, ni, 1000 + 10 * k + extra + ni, satisfied)
        ck = circuit_from_pymodel(cp, cs, z)
        want = cm.witness_map(cp, cs, z)
        assert len(want) == ck.domain_size == (1 << (k + extra if total > 1 else 0))
        got = mont_to_ints(gpu_map(circom, g, ck), cp.r)
        assert got == want, (k, extra, ni)


FREE_TRIPLES = ["pm1_all", "alt_alt_pm1", "impulses", "mirror_alt_half_pm1", "ones_pm1_zeros"]


@pytest.mark.parametrize("tname", FREE_TRIPLES)
@pytest.mark.parametrize("k", [9, 10, 11, 12])
def test_map_free_vectors_equal_model(env, g, orc, k, tname):
    """a and b ARE the named worst-case vectors (constant p - 1, +-1 alternations, impulses; transform_cases): the lazy ranges of
    the fused inverse / forward kernel with this map's pre-scale table, one pass (9, 10) and two (11, 12)"""
    curve, circom, _ = env
    cp = CP[curve]
    va, vb, vc = tc.triple_mont(cp, k, tname, orc)
    ck = tc.free_vector_circuit(curve, k, va, vb, vc)
    cs, z = tc.r1cs_of(ck)
    got = tc.from_mont(gpu_map(circom, g, ck), cp.r)
    assert got == cm.witness_map(cp, cs, z)


# ---------------------------------------------------------------------------------------------------------------------------
# map at size: the -2 identity against the Libsnark map of the same circuit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 19])
def test_map_at_size_is_minus_two_times_shifted_libsnark_quotient(env, g, orc, k):
    curve, circom, libsnark = env
    cp = CP[curve]
    p = cp.r
    ck = orc.syn_circuit(curve, k, 40 + k)
    h_lib = gpu_map(libsnark, g, ck)
    n = 1 << k
    _, rho = cm.roots(cp, n)
    vals, acc = tc.from_mont(h_lib, p), p - 2
    for i in range(n):   # -2 rho^i h[i]
        vals[i] = vals[i] * acc % p
        acc = acc * rho % p
    want = libsnark.ntt(tc.to_mont(vals, p))
    got = gpu_map(circom, g, ck)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d of %d differ, first at %d" % (bad.size, n, bad[0])
    assert got.any()


# ---------------------------------------------------------------------------------------------------------------------------
# keys, proofs
# ---------------------------------------------------------------------------------------------------------------------------
def make_key(prover, orc, g, ck, seed):
    curve = ck.curve
    toxic = orc.rand_fr(curve, seed, 5)
    gens = orc.setup(orc.syn_circuit(curve, 2, 1), 3)[1]
    return prover.generate_parameters_with_qap(mats_of(g, ck), toxic[0], toxic[1], toxic[2], toxic[3], gens["g1gen"], gens["g2gen"], toxic[4])


def public_inputs(ck):
    return [ck.z[i] for i in range(1, ck.num_inputs)]


def test_host_and_device_assignment_agree(g, orc):
    """2^17 + 1 variables: the smallest assignment that g16_prove uploads in more than one piece (two), the row kernel following
    the pieces.  h through g16_witness_map and the proof through g16_prove, host assignment against device assignment"""
    import torch

    curve, k = "bn254", 17
    ck = orc.syn_circuit(curve, k, 31)
    assert ck.num_vars >> 16 >= 2
    z_dev = torch.from_numpy(ck.z.view(np.int64)).cuda()
    r, s = orc.rand_fr(curve, 51, 1)[0], orc.rand_fr(curve, 52, 1)[0]
    with g.Groth16(curve, 0, qap=g.CircomReduction) as prover:
        mats = mats_of(g, ck)
        lb, ctx = prover._ctx.lib, prover._ctx.handle
        dck = prover._ck(mats)
        assert dck.qap == 1 and dck.domain_size == 1 << k
        hs = []
        for on_device, ptr in ((0, ck.z.ctypes.data), (1, z_dev.data_ptr())):
            h = np.zeros((1 << k, 4), dtype=np.uint64)
            lb.check(lb.c.g16_witness_map(ctx, dck.handle, C.c_void_p(ptr), ck.num_vars, on_device, h.ctypes.data_as(C.POINTER(C.c_uint64))))
            hs.append(h)
        assert (hs[0] == hs[1]).all() and hs[0].any()
        pk = orc.synth_pk(ck, 77)
        gp = g.ProvingKey(curve, pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, pk.a_query, pk.b_g1_query, pk.b_g2_query,
                          np.ascontiguousarray(orc.synth_bases(curve, False, 79, 1 << k)), pk.l_query)
        dpk = prover._pk(gp, ck.num_inputs)
        from groth16_amd.binding import ProofC, ptr64
        proofs = []
        for on_device, ptr in ((0, ck.z.ctypes.data), (1, z_dev.data_ptr()), (0, ck.z.ctypes.data)):
            out = ProofC()
            lb.check(lb.c.g16_prove(ctx, dpk.handle, dck.handle, C.c_void_p(ptr), ck.num_vars, on_device, ptr64(r), ptr64(s), C.byref(out)))
            proofs.append(bytes(out))
        assert proofs[0] == proofs[1] == proofs[2]
        tm = prover.timings()
        assert tm["ntt_ms"] > 0 and tm["ntt_ms"] <= tm["witness_map_ms"]


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


@pytest.mark.parametrize("nc", [1 << 4, (1 << 7) - 2, 1 << 10], ids=["2^4", "2^7-2", "2^10"])
def test_setup_prove_verify(env, g, nc):
    """(2^7 - 2 constraints + 2 instance variables: a domain filled exactly)"""
    import random

    curve, circom, _ = env
    p = CP[curve].r
    circuit = Chain(p, nc, 5 + nc)
    rng = random.Random(nc)
    pk, vk = circom.setup(circuit, rng)
    n = 1
    while n < nc + 2:
        n <<= 1
    assert len(pk.h_query) == n
    assert circom.pk_info(pk, 2)["window_bits_h"] > 0    # the n = 2^k bases of h_query as window tables: the merged-plan sort
    pvk = circom.prepare_verifying_key(vk)
    x = ints_to_mont([circuit.u[-1]], p, 4)
    wrong = ints_to_mont([(circuit.u[-1] + 1) % p], p, 4)
    for proof in (circom.prove(pk, circuit, rng), circom.create_proof_no_zk(circuit, pk)):     # r = s = 0 too
        assert circom.verify_proof(pvk, proof, [x[0]])
        assert g.verify_proof_host(curve, vk, proof, [x[0]])
        assert not circom.verify_proof(pvk, proof, [wrong[0]])
        assert not g.verify_proof_host(curve, vk, proof, [wrong[0]])
    pvk.close()
    circom.evict()


def test_libsnark_key_with_circom_circuit(env, g, orc):
    """the Libsnark key of the same circuit is one h base short: the length rules pass it (n - 1 <= n) and the proof is rejected;
    the other way round (Circom key, Libsnark circuit) likewise"""
    curve, circom, libsnark = env
    ck = orc.syn_circuit(curve, 6, 9)
    mats = mats_of(g, ck)
    r, s = orc.rand_fr(curve, 61, 1)[0], orc.rand_fr(curve, 62, 1)[0]
    pk_lib, pk_cir = make_key(libsnark, orc, g, ck, 900), make_key(circom, orc, g, ck, 900)
    assert len(pk_lib.h_query) == 63 and len(pk_cir.h_query) == 64
    for name in ("a_query", "b_g2_query", "l_query", "gamma_abc_g1", "delta_g2"):     # only h_query depends on the reduction
        assert (getattr(pk_lib, name) == getattr(pk_cir, name)).all(), name
    x = public_inputs(ck)
    for prover, good, bad in ((circom, pk_cir, pk_lib), (libsnark, pk_lib, pk_cir)):
        ok = prover.create_proof_with_reduction_and_matrices(good, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z)
        assert g.verify_proof_host(curve, good, ok, x)
        mixed = prover.create_proof_with_reduction_and_matrices(bad, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z)
        assert not g.verify_proof_host(curve, bad, mixed, x)
        prover.evict()


@pytest.mark.parametrize("mode", ["base", "bucket"])
def test_sharded_proof_equals_single(env, g, orc, mode):
    """two ranks on one GPU (the map replicated): prove_partial x 2 + prove_finalize, byte for byte g16_prove's proof"""
    curve, circom, _ = env
    ck = orc.syn_circuit(curve, 9, 3)
    mats = mats_of(g, ck)
    pk = make_key(circom, orc, g, ck, 910)
    for r, s in ((orc.rand_fr(curve, 31, 1)[0], orc.rand_fr(curve, 32, 1)[0]), (np.zeros(4, dtype=np.uint64), orc.rand_fr(curve, 33, 1)[0])):
        want = circom.create_proof_with_reduction_and_matrices(pk, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z)
        shard = (lambda i: (i, 2, "bucket")) if mode == "bucket" else (lambda i: (i, 2))
        parts = [circom.prove_partial(pk, mats, ck.z, shard(i), skip_b_g1=not r.any()) for i in range(2)]
        proof = circom.prove_finalize(pk, ck.num_inputs, parts, r, s, shard(0))
        assert proof.flat().tobytes() == want.flat().tobytes()
        assert g.verify_proof_host(curve, pk, proof, public_inputs(ck))
    circom.evict()


def test_window_table_key_two_classes(g, orc, monkeypatch):
    """BN254, a key from g16_generate_parameters_qap held as window tables with c = 17 (two classes of the merged plan) over a
    2^16-base h_query, one proof, checked by the verifier.

    There is no separate 2^20-point case, and none is missing.  The issue asked for "the smallest size for which g16_pk_get_info
    reports window_bits_h > 0" and read the header (include/g16_mi355x.h, g16_pk_load) as putting that at 2^20 points; that reading
    was wrong.  The header's 2^20 is where the window size reaches c = 20 / W = 13, not where tables begin: keys are held as window
    tables at EVERY size by default, which test_setup_prove_verify asserts from 2^4 up (window_bits_h > 0).
    So the smallest such size is already covered there, 2^k-base h_query on the merged plan included, and what this test adds is
    the one plan shape those sizes do not reach: more than one class."""
    monkeypatch.setenv("G16_MSM_PRECOMP_WINDOW", "17")
    curve, k = "bn254", 16
    ck = orc.syn_circuit(curve, k, 21)
    r, s = orc.rand_fr(curve, 71, 1)[0], orc.rand_fr(curve, 72, 1)[0]
    with g.Groth16(curve, 0, qap=g.CircomReduction) as prover:
        pk = make_key(prover, orc, g, ck, 920)
        assert len(pk.h_query) == 1 << k
        info = prover.pk_info(pk, ck.num_inputs)
        assert info["window_bits_h"] == 17 and info["table_fallback"] == 0
        proof = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats_of(g, ck), ck.num_inputs, ck.num_constraints, ck.z)
        pvk = prover.prepare_verifying_key(pk)
        assert prover.verify_proof(pvk, proof, public_inputs(ck))
        assert not prover.verify_proof(pvk, proof, [r])


def test_pipelined_prover_and_block_order_keys(g, orc):
    """The two reductions are sibling classes (neither is a subclass of the other); PipelinedProver(qap=CircomReduction) gives the
    proof Groth16(qap=CircomReduction) gives; the block-order key shards of the distributed witness map (dist_h: they take
    n = len(h_query) + 1, the Libsnark length) raise on a Circom prover instead of gathering a wrong order"""
    assert not issubclass(g.CircomReduction, g.LibsnarkReduction) and not issubclass(g.LibsnarkReduction, g.CircomReduction)
    curve = "bn254"
    ck = orc.syn_circuit(curve, 6, 4)
    mats = mats_of(g, ck)
    r, s = orc.rand_fr(curve, 81, 1)[0], orc.rand_fr(curve, 82, 1)[0]
    with g.Groth16(curve, 0, qap=g.CircomReduction) as prover:
        pk = make_key(prover, orc, g, ck, 930)
        want = prover.create_proof_with_reduction_and_matrices(pk, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z)
        with pytest.raises(ValueError):
            prover.pk_info(pk, ck.num_inputs, (0, 2), dist_h=True)
        with pytest.raises(ValueError):
            prover.prove_partial_prepare(pk, mats, 0, ck.num_vars, (0, 2))
        with pytest.raises(ValueError):
            prover.prove_partial_h(pk, mats, ck.z, (0, 2), 0, 0)
        with pytest.raises(ValueError):
            prover.prove_finalize(pk, ck.num_inputs, [], r, s, (0, 2), dist_h=True)
    with g.PipelinedProver(curve, 0, qap=g.CircomReduction) as pipe:
        got = [pipe.submit(pk, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z) for _ in range(2)]
        for fut in got:
            assert fut.result(timeout=120).flat().tobytes() == want.flat().tobytes()
    assert g.verify_proof_host(curve, pk, want, public_inputs(ck))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(g, orc):
    from groth16_amd.binding import CsrViewC, lib, ptr32, ptr64

    curve = "bn254"
    ck = orc.syn_circuit(curve, 6, 2)
    lb = lib()
    views = (CsrViewC * 3)(*[CsrViewC(ptr64(m.row_ptr), ptr32(m.col), ptr64(m.val)) for m in ck.abc])
    with g.Groth16(curve, 0, qap=g.CircomReduction) as prover:
        dck = prover._ck(mats_of(g, ck))
        dwm = C.c_void_p()
        assert lb.c.g16_dwm_create(prover._ctx.handle, dck.handle, 0, 2, C.byref(dwm)) == BAD_ARG
        assert not dwm.value
        bad = C.c_void_p()
        assert lb.c.g16_circuit_load_qap(prover._ctx.handle, views, ck.num_inputs, ck.num_constraints, ck.num_vars, 2, C.byref(bad)) == BAD_ARG
        # abc[2] all-NULL is a Circom circuit all the same
        two = (CsrViewC * 3)(views[0], views[1], CsrViewC(None, None, None))
        noc = C.c_void_p()
        assert lb.c.g16_circuit_load_qap(prover._ctx.handle, two, ck.num_inputs, ck.num_constraints, ck.num_vars, 1, C.byref(noc)) == 0
        assert lb.c.g16_circuit_qap(noc) == 1
        lb.c.g16_circuit_free(noc)
    with g.Groth16(curve, [0, 0]) as multi:
        out = C.c_void_p()
        assert lb.c.g16_circuit_load_qap(multi._ctx.handle, views, ck.num_inputs, ck.num_constraints, ck.num_vars, 1, C.byref(out)) == BAD_ARG
        assert not out.value
        assert lb.c.g16_circuit_load_qap(multi._ctx.handle, views, ck.num_inputs, ck.num_constraints, ck.num_vars, 0, C.byref(out)) == 0
        lb.c.g16_circuit_free(out)
