"""GPU tier: a serialized proving key loaded on the device (g16_decode_points, g16_pk_load_bytes, Groth16.load_proving_key_bytes).

Points: the whole case list of key_bytes_cases tiled to 130 points (two waves and a 2-lane tail), every encoding and validation
level, against the host twin and the model's labels.  Keys: the smallest oracle circuit whose five queries each exceed 128 points
(syn_circuit at k = 8: 257 / 257 / 257 / 255 / 255 points; its CPU setup takes about a second), loaded with G16_PK_BYTES_CHUNK=64 so
that every query spans several chunks -- honest keys against the host path (same pk_info, bit-equal proofs), corrupted keys
against the exact section, index and reason of the first bad point in file order."""
import ctypes as C

import numpy as np
import pytest

import key_bytes_cases as kc
import pymodel as pm
from subgroup_cases import NAMES

pytestmark = pytest.mark.gpu

K = 8
SPLICE = (0, 63, 64, -1)   # identities at the first index, either side of a chunk border and at the last index of every query
QUERIES = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")
INVALID_DATA = 9


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available()
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module")
def provers(g):
    ps = {name: g.Groth16(name, device=0) for name in NAMES}
    yield ps
    for p in ps.values():
        p.close()


@pytest.fixture(scope="module")
def env(g, orc, provers):
    """per curve: the circuit, r, s, two keys (as the oracle made it; with identities spliced in), their bytes in both encodings, and
    for each key what the HOST path gives: the key back from its bytes, its pk_info and the proof under fixed r, s"""
    import groth16_amd.serialize as ser

    out = {}
    for name in NAMES:
        ck = orc.syn_circuit(name, K, 31)
        pk, ex = orc.setup(ck, 32)
        mats = g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints, *[(m.row_ptr, m.col, m.val) for m in ck.abc])
        r, s = orc.rand_fr(name, 33, 1)[0], orc.rand_fr(name, 34, 1)[0]
        e = dict(ck=ck, mats=mats, r=r, s=s, keys={})
        for kind in ("plain", "spliced"):
            q = {f: np.array(getattr(pk, f), copy=True) for f in QUERIES}
            if kind == "spliced":
                for f in QUERIES:
                    assert len(q[f]) > 128
                    q[f][list(SPLICE)] = 0
            key = g.ProvingKey(name, pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, q["a_query"], q["b_g1_query"], q["b_g2_query"],
                               q["h_query"], q["l_query"], ex["gamma_g2"][None, :], ex["gamma_abc"])
            data = {c: ser.proving_key_to_bytes(name, key, c) for c in (True, False)}
            back, used = ser.proving_key_from_bytes(name, data[True], True, validate=2)
            assert used == len(data[True])
            for f in QUERIES:
                assert back.__dict__[f].tobytes() == q[f].tobytes()
            prover = provers[name]
            proof = prover.create_proof_with_reduction_and_matrices(back, r, s, mats, ck.num_inputs, ck.num_constraints, ck.z)
            e["keys"][kind] = dict(key=key, data=data, host_proof=proof, host_info=prover.pk_info(back, ck.num_inputs))
            prover.evict_pk(back)
        out[name] = e
    return out


def load(g, prover, data, compressed, validate):
    """g16_pk_load_bytes through the C ABI: (status, handle, info)"""
    from groth16_amd.binding import PkBytesInfoC

    info, handle = PkBytesInfoC(), C.c_void_p(0xDEAD)
    rc = g.lib().c.g16_pk_load_bytes(prover._ctx.handle, data, len(data), int(compressed), validate, C.byref(handle), C.byref(info),
                                     C.sizeof(info))
    return rc, handle, info


def prove_with_handle(g, prover, e, handle):
    from groth16_amd.groth16 import _DevicePk

    dpk = _DevicePk.from_handle(prover._ctx, handle)
    try:
        ck = e["ck"]
        L = g.FQ_LIMBS[prover.curve]
        out = g.binding.ProofC()
        z = np.ascontiguousarray(ck.z)
        dck = prover._ck(e["mats"])
        lb = g.lib()
        lb.check(lb.c.g16_prove(prover._ctx.handle, dpk.handle, dck.handle, z.ctypes.data, z.shape[0], 0, g.binding.ptr64(np.ascontiguousarray(e["r"])),
                                g.binding.ptr64(np.ascontiguousarray(e["s"])), C.byref(out)))
        return g.Proof(np.array(out.a[: 2 * L], dtype=np.uint64), np.array(out.b[: 4 * L], dtype=np.uint64),
                       np.array(out.c[: 2 * L], dtype=np.uint64)), dpk.info()
    finally:
        dpk.close()


# ---- points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("validate", kc.VALIDATE)
def test_decode_points_match_host_and_model(g, provers, name, g2, compressed, validate):
    labels, encs, status, points = kc.cases(name, g2, compressed)
    idx = np.arange(130) % len(encs)
    assert len(encs) < 130
    data = kc.blob(encs, idx)
    pts, st = provers[name].decode_points(data, g2, compressed, validate)
    host_pts, host_st = g.decode_points_host(name, data, g2, compressed, validate)
    assert st.tobytes() == host_st.tobytes(), [(labels[i], int(a), int(b)) for i, a, b in zip(idx, st, host_st) if a != b]
    assert pts.tobytes() == host_pts.tobytes()
    assert st.tolist() == status[validate][idx].tolist()
    assert pts.tobytes() == points[validate][idx].tobytes()


def test_decode_points_empty(g, provers):
    pts, st = provers["bn254"].decode_points(b"", False, False, 2)
    assert pts.shape == (0, 8) and st.shape == (0,)


# ---- honest keys ------------------------------------------------------------------------------------------------------------------
def check_honest(g, prover, e, kind, compressed, validate):
    k = e["keys"][kind]
    data = k["data"][compressed]
    rc, handle, info = load(g, prover, data, compressed, validate)
    assert rc == 0, (rc, g.lib().c.g16_last_error())
    offs, total = kc.section_offsets(prover.curve, e["ck"], compressed)
    assert info.consumed == total == len(data) and info.bad_section == -1 and info.n_bad == 0
    assert info.counts() == {sec: offs[sec][3] for sec in kc.SECTIONS}
    proof, pk_info = prove_with_handle(g, prover, e, handle)
    assert pk_info == k["host_info"]
    assert proof.flat().tobytes() == k["host_proof"].flat().tobytes()   # bit-equal with the key loaded through the host path
    return proof


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("validate", kc.VALIDATE)
def test_honest_key_chunked(g, provers, env, monkeypatch, name, compressed, validate):
    monkeypatch.setenv("G16_PK_BYTES_CHUNK", "64")
    prover, e = provers[name], env[name]
    check_honest(g, prover, e, "spliced", compressed, validate)
    proof = check_honest(g, prover, e, "plain", compressed, validate)
    ck = e["ck"]
    pvk = prover.prepare_verifying_key(e["keys"]["plain"]["key"])
    assert prover.verify_proof(pvk, proof, ck.z[1: ck.num_inputs])


@pytest.mark.parametrize("name", NAMES)
def test_honest_key_default_chunk(g, provers, env, monkeypatch, name):
    monkeypatch.delenv("G16_PK_BYTES_CHUNK", raising=False)
    check_honest(g, provers[name], env[name], "spliced", True, 2)
    monkeypatch.setenv("G16_PK_BYTES_CHUNK", "1")   # below the minimum: 64 is used
    check_honest(g, provers[name], env[name], "spliced", False, 2)


# ---- bad keys ---------------------------------------------------------------------------------------------------------------------
# every kind of position the issue names, spread over the sections; b_g2_query takes the G2 case list
POSITIONS = [("a_query", 0), ("b_g1_query", -1), ("b_g2_query", 63), ("h_query", 64), ("l_query", -1), ("l_query", 0), ("alpha_g1", 0),
             ("gamma_abc_g1", 1)]


def failing_cases(name, g2, compressed, validate=2):
    """(label, encoding, status) of the case list's failures, one per kind (the +1 and signed variants repeat their kind)"""
    labels, encs, status, _ = kc.cases(name, g2, compressed)
    return [(l, e, int(s)) for l, e, s in zip(labels, encs, status[validate]) if s != 1 and not l.endswith(("_plus_1", "_signed"))]


def corrupt(data, offs, section, index, enc):
    _, first, size, count = offs[section]
    at = first + (index % count) * size
    assert len(enc) == size
    return data[:at] + enc + data[at + size:], index % count


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("section,index", POSITIONS, ids=[f"{s}[{i}]" for s, i in POSITIONS])
def test_bad_key_names_the_point(g, provers, env, monkeypatch, name, compressed, section, index):
    monkeypatch.setenv("G16_PK_BYTES_CHUNK", "64")
    prover, e = provers[name], env[name]
    data = e["keys"]["plain"]["data"][compressed]
    offs, _ = kc.section_offsets(name, e["ck"], compressed)
    kinds = failing_cases(name, section in kc.G2_SECTIONS, compressed)
    torsion = not (name == "bn254" and section not in kc.G2_SECTIONS)   # BN254's G1 is the whole curve
    assert {s for _, _, s in kinds} == {0} | (set() if compressed else {2}) | ({3} if torsion else set())
    for label, enc, status in kinds:
        bad, at = corrupt(data, offs, section, index, enc)
        rc, handle, info = load(g, prover, bad, compressed, 2)
        assert rc == INVALID_DATA and handle.value is None, (label, rc)
        assert (kc.SECTIONS[info.bad_section], info.bad_index, info.bad_reason, info.n_bad) == (section, at, status, 1), label
        assert info.consumed == 0
        # no state leaks: the same context loads the honest bytes and proves the same proof
        check_honest(g, prover, e, "plain", compressed, 2)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
def test_first_bad_point_in_file_order(g, provers, env, monkeypatch, name, compressed):
    monkeypatch.setenv("G16_PK_BYTES_CHUNK", "64")
    prover, e = provers[name], env[name]
    data = e["keys"]["plain"]["data"][compressed]
    offs, _ = kc.section_offsets(name, e["ck"], compressed)
    g1, g2 = failing_cases(name, False, compressed), failing_cases(name, True, compressed)
    # two queries: the earlier one in file order is reported, whichever the GPU met first
    bad, _ = corrupt(data, offs, "h_query", 5, g1[0][1])
    bad, at = corrupt(bad, offs, "b_g2_query", 200, g2[-1][1])
    rc, handle, info = load(g, prover, bad, compressed, 2)
    assert rc == INVALID_DATA and handle.value is None
    assert (kc.SECTIONS[info.bad_section], info.bad_index, info.bad_reason, info.n_bad) == ("b_g2_query", 200, g2[-1][2], 2)
    # one query, three chunks: the lowest index, with ITS status
    bad, _ = corrupt(data, offs, "l_query", 130, g1[0][1])
    bad, _ = corrupt(bad, offs, "l_query", 70, g1[-1][1])
    bad, _ = corrupt(bad, offs, "l_query", 7, g1[1][1])
    rc, handle, info = load(g, prover, bad, compressed, 2)
    assert rc == INVALID_DATA and (kc.SECTIONS[info.bad_section], info.bad_index, info.bad_reason, info.n_bad) == ("l_query", 7, g1[1][2], 3)
    # the head comes before every query
    bad, _ = corrupt(data, offs, "a_query", 0, g1[0][1])
    bad, _ = corrupt(bad, offs, "delta_g1", 0, g1[1][1])
    rc, handle, info = load(g, prover, bad, compressed, 2)
    assert rc == INVALID_DATA and (kc.SECTIONS[info.bad_section], info.bad_index, info.bad_reason, info.n_bad) == ("delta_g1", 0, g1[1][2], 2)
    check_honest(g, prover, e, "plain", compressed, 2)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
def test_torsion_point_passes_without_the_subgroup_check(g, provers, env, monkeypatch, name, compressed):
    monkeypatch.setenv("G16_PK_BYTES_CHUNK", "64")
    prover, e = provers[name], env[name]
    data = e["keys"]["plain"]["data"][compressed]
    offs, _ = kc.section_offsets(name, e["ck"], compressed)
    section, g2 = ("b_g2_query", True) if name == "bn254" else ("h_query", False)   # BN254's G1 has no such point
    label, enc, status = [c for c in failing_cases(name, g2, compressed) if c[0].startswith("order")][0]
    assert status == 3
    bad, at = corrupt(data, offs, section, 64, enc)
    for validate in (0, 1):
        rc, handle, info = load(g, prover, bad, compressed, validate)
        assert rc == 0 and info.bad_section == -1 and info.n_bad == 0
        g.lib().c.g16_pk_free(handle)
    rc, handle, info = load(g, prover, bad, compressed, 2)
    assert rc == INVALID_DATA and handle.value is None
    assert (kc.SECTIONS[info.bad_section], info.bad_index, info.bad_reason, info.n_bad) == (section, 64, 3, 1)
    check_honest(g, prover, e, "plain", compressed, 2)


def test_truncated_key_and_multi_device_context(g, provers, env):
    prover, e = provers["bn254"], env["bn254"]
    data = e["keys"]["plain"]["data"][True]
    rc, handle, info = load(g, prover, data[:-1], True, 2)
    assert rc == 2 and handle.value is None and kc.SECTIONS[info.bad_section] == "l_query" and info.bad_reason == 4
    with g.Groth16("bn254", device=[0, 0]) as multi:
        rc, handle, info = load(g, multi, data, True, 2)
        assert rc == 3 and handle.value is None
        assert b"one GPU" in g.lib().c.g16_last_error()
    check_honest(g, prover, e, "plain", True, 2)


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
class Product:
    """a * b = c, six times over; c public"""

    def __init__(self, a=None, b=None):
        self.a, self.b = a, b

    def generate_constraints(self, cs):
        from groth16_amd import lc

        a = cs.new_witness_variable(lambda: self.a)
        b = cs.new_witness_variable(lambda: self.b)
        c = cs.new_input_variable(lambda: None if self.a is None or self.b is None else self.a * self.b)
        for _ in range(6):
            cs.enforce_constraint(lc() + a, lc() + b, lc() + c)


@pytest.mark.parametrize("name", NAMES)
def test_python_surface(g, name):
    import random

    import groth16_amd.serialize as ser
    from groth16_amd.r1cs import synthesize
    from helpers import ints_to_mont

    rng = random.Random(77)
    cp = pm.CURVES[name]
    with g.Groth16(name, device=0) as prover:
        pk, vk = prover.setup(Product(), rng)
        data = ser.proving_key_to_bytes(name, pk, compressed=True)
        dkey = prover.load_proving_key_bytes(data + b"tail")
        assert isinstance(dkey, g.DeviceProvingKey) and dkey.resident and dkey.consumed == len(data)
        assert dkey.counts["a_query"] == len(pk.a_query) and dkey.counts["h_query"] == len(pk.h_query) and dkey.counts["alpha_g1"] == 1
        for f in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2", "gamma_abc_g1"):
            assert np.asarray(getattr(dkey, f)).tobytes() == np.asarray(getattr(pk, f)).tobytes(), f
        assert prover.pk_info(dkey, 2) == prover.pk_info(pk, 2)
        public = ints_to_mont([21], cp.r, 4)
        pvk = prover.prepare_verifying_key(dkey)
        proof = prover.prove(dkey, Product(3, 7), rng)
        assert prover.verify_proof(pvk, proof, public)
        assert prover.verify_proof(pvk, prover.rerandomize_proof(dkey, proof, rng), public)
        zk = prover.create_proof_no_zk(Product(3, 7), dkey)
        assert zk == prover.create_proof_no_zk(Product(3, 7), pk) == prover.create_proof_with_reduction_no_zk(Product(3, 7), dkey)
        # what reads the query arrays on the host says so
        cs_m = synthesize(name, Product(3, 7), False)
        mats, z = cs_m.to_matrices(), cs_m.full_assignment()
        for call in (lambda: prover.prove_partial(dkey, mats, z, (0, 1)), lambda: prover.pk_info(dkey, 2, shard=(0, 2)),
                     lambda: prover.prove_partial_h(dkey, mats, z, (0, 1), 0, 0), lambda: prover.prove_finalize(dkey, 2, [], zk.a, zk.a),
                     lambda: g.ShardedProver(prover, dkey, mats, 0, 1), lambda: g.finalize_host(name, dkey, [], zk.a, zk.a),
                     lambda: ser.proving_key_to_bytes(name, dkey)):
            with pytest.raises(TypeError, match="query arrays on the host"):
                call()
        # a bad key: the exception names the point
        size = ser.point_size(name, False, True)
        h0 = len(data) - (8 + len(pk.l_query) * size) - len(pk.h_query) * size   # the file ends with Vec h_query, Vec l_query
        bad = bytearray(data)
        bad[h0: h0 + size] = [c for c in failing_cases(name, False, True) if c[0] == "no_point"][0][1]
        with pytest.raises(g.InvalidData) as ei:
            prover.load_proving_key_bytes(bytes(bad))
        assert (ei.value.section, ei.value.index, ei.value.reason, ei.value.n_bad) == ("h_query", 0, 0, 1)
        # eviction frees the tables; the key cannot prove afterwards, and says so
        prover.evict_pk(dkey)
        assert not dkey.resident
        with pytest.raises(ValueError, match="evicted"):
            prover.prove(dkey, Product(3, 7), rng)
        again = prover.load_proving_key_bytes(data, compressed=True, validate=0)
        assert prover.verify_proof(pvk, prover.prove(again, Product(2, 5), rng), ints_to_mont([10], cp.r, 4))
    assert not again.resident   # close() frees what load_proving_key_bytes made
