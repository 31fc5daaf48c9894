"""GPU tier: whole proofs whose G1 MSMs reach the heavy-bucket stage INSIDE the prover's own batching, over every branch of the schedule
prove_partial chooses (csrc/prover.hpp), compared bit for bit with the CPU oracle's proof on the same key.

The other proof tests leave the batched reductions' per-MSM indexing unobserved: l, a and b_g1 share the witness sort (one heavy list,
one set of slot offsets), h is uniformly random (no heavy bucket), and the one all-equal witness in the suite proves on a key that is
the identity almost everywhere.  Here the key is made of random bases (orc.synth_pk), the circuit is small (2^11), and the witness is
  equal     every value the same full-width scalar: each window's digit falls into ONE bucket of a thousand entries
  boolean   0 / 1 with a few full-width values: half the witness sits in bucket 0 of the merged windows
  three     three distinct full-width values
with G16_MSM_SEGMENT=8 and G16_MSM_PRECOMP_WINDOW=9 (256 buckets, parts of at most 8 entries), so that such a bucket has far more
than HEAVY_PARTS partial sums.  That is a precondition, asserted with the sort lab on the same scalars, window and environment -- its
heavy count, and the bucket-part rule on its histogram: ceil(largest bucket / 8) > HEAVY_PARTS -- not assumed; h's count is printed.
h's sort has another heavy list (none, on these inputs) and other slot offsets than the witness sort's, inside one launch of every
reduction kernel.

After each call g16_timings.g1_pass_launches is compared with the rule the header and prover.hpp document, derived from the case's own
conditions (expected_launches), never copied from a run.  Every proof runs twice on one context: stale events or buffers of the first
must not satisfy the second."""
import dataclasses
import random

import numpy as np
import pytest

import pymodel as pm
import reduce_cases as rc
from helpers import ints_to_mont

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
CP = {"bls12_381": pm.BLS12_381, "bn254": pm.BN254}
POPULATIONS = ["equal", "boolean", "three"]
K = 11         # a third of the witness in one of three shards, a third of that per value of "three": 227 entries, 29 parts
WINDOW, LMAX = 9, 8
ENV = {"G16_MSM_SEGMENT": str(LMAX), "G16_MSM_PRECOMP_WINDOW": str(WINDOW)}
SHARDS = 3


def mats_of(g, ck):
    return g.ConstraintMatrices(ck.num_inputs, ck.num_vars - ck.num_inputs, ck.num_constraints, *[(m.row_ptr, m.col, m.val) for m in ck.abc])


def pk_of(g, pk):
    return g.ProvingKey(pk.curve, pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, pk.a_query, pk.b_g1_query, pk.b_g2_query,
                        pk.h_query, pk.l_query)


def uneven_shard_ranges(m, w, h_len, num_inputs, idx, cnt):
    """groth16.shard_ranges cuts l where a is cut, so that every shard's l MSM reuses the witness sort.  Here l is cut evenly on its
    own: any partition of the five queries sums to the same proof, and a shard whose l range is not inside its a range makes the prover
    sort l separately (l_covered false)."""
    return dict(a=(m * idx // cnt, m * (idx + 1) // cnt), l=(w * idx // cnt, w * (idx + 1) // cnt), h=(h_len * idx // cnt, h_len * (idx + 1) // cnt))


def l_covered(rg, nin):
    """prover.hpp: l's scalars aux[j] = assignment[j + nin - 1] lie inside the witness sort's range, or there are none"""
    (a_lo, a_hi), (l_lo, l_hi) = rg["a"], rg["l"]
    return l_hi == l_lo or (l_lo + nin - 1 >= a_lo and l_hi + nin - 1 <= a_hi)


def expected_launches(n_g1_msms, covered, h_external, plans_match, env):
    """g16_timings.g1_pass_launches by the documented rule: MSMs that are ready together share one launch -- a and b_g1 always, l when
    it reuses the witness sort (else its own sort and launch come first), h when it is supplied from outside and its plan matches
    (G16_PASS_H_IN_BATCH=0 splits it off again); on one GPU h follows alone.  G16_PASS_NO_BATCH: one launch per MSM."""
    if "G16_PASS_NO_BATCH" in env:
        return n_g1_msms
    h_in_batch = h_external and plans_match and env.get("G16_PASS_H_IN_BATCH", "1") != "0"
    return (0 if covered else 1) + (1 if h_in_batch else 2)


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module", params=CURVES)
def world(request, g, orc):
    """one context, circuit and random-bases key per curve, loaded with the window and segment length above in the environment"""
    import groth16_amd.groth16 as gmod

    curve = request.param
    mp = pytest.MonkeyPatch()
    for k_, v in ENV.items():
        mp.setenv(k_, v)
    mp.setattr(gmod, "shard_ranges", uneven_shard_ranges)
    ck = orc.syn_circuit(curve, K, 31)
    pk = orc.synth_pk(ck, 32)
    prover = g.Groth16(curve, 0)
    w = dict(curve=curve, prover=prover, ck=ck, pk=pk, gp=pk_of(g, pk), gm=mats_of(g, ck), cases={},
             r=orc.rand_fr(curve, 33, 1)[0], s=orc.rand_fr(curve, 34, 1)[0])
    yield w
    prover.close()
    mp.undo()


def case(world, orc, population):
    """the circuit with its witness overwritten (proved as given, by the oracle too), the oracle's h and its proofs for r != 0 and r = 0"""
    if population not in world["cases"]:
        curve, ck0 = world["curve"], world["ck"]
        cp = CP[curve]
        rng = random.Random("proof schedule/%s/%s" % (curve, population))
        full = lambda: rng.randrange(cp.r >> 1, cp.r)   # noqa: E731
        n = ck0.num_vars - 1
        if population == "equal":
            vals = [full()] * n
        elif population == "boolean":
            vals = [rng.randrange(2) for _ in range(n)]
            for i in rng.sample(range(n), 5):
                vals[i] = full()
        else:
            three = [full(), full(), full()]
            assert len(set(three)) == 3
            vals = [three[rng.randrange(3)] for _ in range(n)]
        z = ck0.z.copy()
        z[1:] = ints_to_mont(vals, cp.r, 4)
        ck = dataclasses.replace(ck0, z=np.ascontiguousarray(z))
        zero = np.zeros(4, dtype=np.uint64)
        world["cases"][population] = dict(ck=ck, h=orc.witness_map(ck), want=orc.prove(world["pk"], ck, world["r"], world["s"])[0],
                                          want_r0=orc.prove(world["pk"], ck, zero, world["s"])[0])
    return world["cases"][population]


def sort_layout(world, scalars):
    """sort_scalars on these scalars with the key's window and the environment of this module, through the sort lab"""
    from groth16_amd import binding

    prover = world["prover"]
    status, res = binding.msm_sort_lab(prover._ctx.lib, prover._ctx.handle, np.ascontiguousarray(scalars), merged_c=WINDOW)
    assert status == 0, status
    assert res["merged"] == 1 and res["c"] == WINDOW and res["Lmax"] == LMAX, res
    res["largest"] = int(np.diff(res["offsets"].astype(np.int64)).max()) if len(scalars) else 0
    return res


def require_heavy(res, what):
    assert res["heavy"][0] > 0, "%s: the sort lists no heavy bucket; the test would not reach the heavy stage" % what
    assert -(-res["largest"] // LMAX) > rc.HEAVY_PARTS, "%s: largest bucket %d entries: not more than HEAVY_PARTS parts of %d" % (what, res["largest"], LMAX)


def same_layout(x, y):
    return all(x[k] == y[k] for k in ("B", "groups", "Lmax", "merged"))


def preconditions(world, cs, rg, h_scalars, what):
    """the witness sort of this range (and l's own, where it has one) reaches the heavy stage; returns whether h's plan matches"""
    ck = cs["ck"]
    nin = ck.num_inputs
    (a_lo, a_hi), (l_lo, l_hi) = rg["a"], rg["l"]
    zs = sort_layout(world, ck.z[1 + a_lo:1 + a_hi])
    require_heavy(zs, what + ", witness sort")
    if not l_covered(rg, nin):
        require_heavy(sort_layout(world, ck.z[nin + l_lo:nin + l_hi]), what + ", l's own sort")
    hs = sort_layout(world, h_scalars)
    print("%s: heavy buckets: witness sort %d (largest bucket %d entries), h sort %d (largest %d)" % (
        what, zs["heavy"][0], zs["largest"], hs["heavy"][0], hs["largest"]))
    return same_layout(zs, hs)


WHOLE = [("no_knob", {}, False), ("no_batch", {"G16_PASS_NO_BATCH": "1"}, False), ("concurrent_0", {"G16_PASS_CONCURRENT": "0"}, False),
         ("concurrent_1", {"G16_PASS_CONCURRENT": "1"}, False), ("map_under_passes", {"G16_MAP_UNDER_PASSES": "1"}, False),
         ("upload_in_one_copy", {"G16_UPLOAD_CHUNKED": "0"}, False), ("r_zero_skips_b_g1", {}, True)]


@pytest.mark.parametrize("knob", WHOLE, ids=[k[0] for k in WHOLE])
@pytest.mark.parametrize("population", POPULATIONS)
def test_whole_key(world, orc, g, population, knob, monkeypatch):
    _, env, r_zero = knob
    cs = case(world, orc, population)
    ck, prover = cs["ck"], world["prover"]
    rg = uneven_shard_ranges(ck.num_vars - 1, ck.num_vars - ck.num_inputs, len(world["pk"].h_query), ck.num_inputs, 0, 1)
    assert l_covered(rg, ck.num_inputs)
    match = preconditions(world, cs, rg, cs["h"][:len(world["pk"].h_query)], "%s, %s, whole key" % (world["curve"], population))
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    r = np.zeros(4, dtype=np.uint64) if r_zero else world["r"]
    want = cs["want_r0"] if r_zero else cs["want"]
    expect = expected_launches(3 if r_zero else 4, True, False, match, env)
    for it in range(2):
        proof = prover.create_proof_with_reduction_and_matrices(world["gp"], r, world["s"], world["gm"], ck.num_inputs, ck.num_constraints, ck.z)
        assert (proof.flat() == want).all(), "proof %d differs from the oracle's" % it
        assert prover.timings()["g1_pass_launches"] == expect, (it, prover.timings()["g1_pass_launches"], expect)


@pytest.mark.parametrize("population", POPULATIONS)
def test_base_range_shards_with_l_sorted_separately(world, orc, g, population):
    cs = case(world, orc, population)
    ck, prover, gp, gm = cs["ck"], world["prover"], world["gp"], world["gm"]
    nin = ck.num_inputs
    ranges = [uneven_shard_ranges(ck.num_vars - 1, ck.num_vars - nin, len(world["pk"].h_query), nin, i, SHARDS) for i in range(SHARDS)]
    covered = [l_covered(rg, nin) for rg in ranges]
    assert not all(covered), "every shard's l range lies inside its a range: l is never sorted separately"
    expect = []
    for i, rg in enumerate(ranges):
        match = preconditions(world, cs, rg, cs["h"][rg["h"][0]:rg["h"][1]], "%s, %s, shard %d of %d" % (world["curve"], population, i, SHARDS))
        expect.append(expected_launches(4, covered[i], False, match, {}))
    assert 3 in expect   # l, then a and b_g1, then h
    for it in range(2):
        parts = []
        for i in range(SHARDS):
            parts.append(prover.prove_partial(gp, gm, ck.z, (i, SHARDS)))
            assert prover.timings()["g1_pass_launches"] == expect[i], (it, i, prover.timings()["g1_pass_launches"], expect[i])
        proof = prover.prove_finalize(gp, nin, parts, world["r"], world["s"], (0, SHARDS))
        assert (proof.flat() == cs["want"]).all(), "proof %d differs from the oracle's" % it


@pytest.mark.parametrize("knob", [("no_knob", {}), ("h_not_in_batch", {"G16_PASS_H_IN_BATCH": "0"})], ids=lambda k: k[0])
@pytest.mark.parametrize("population", POPULATIONS)
def test_external_h(world, orc, g, population, knob, monkeypatch):
    """h from the distributed witness map of one rank, enqueued on the library's witness-map stream with no host synchronisation and
    g16_prove_partial_h right behind it: l, a, b_g1 and h go as ONE launch, and one launch of every reduction kernel with all four
    inside (heavy_done = false)"""
    import torch
    from groth16_amd.groth16 import DistributedWitnessMap

    _, env = knob
    cs = case(world, orc, population)
    ck, prover, gp, gm = cs["ck"], world["prover"], world["gp"], world["gm"]
    rg = uneven_shard_ranges(ck.num_vars - 1, ck.num_vars - ck.num_inputs, len(world["pk"].h_query), ck.num_inputs, 0, 1)
    match = preconditions(world, cs, rg, cs["h"][:len(world["pk"].h_query)], "%s, %s, external h" % (world["curve"], population))
    assert match   # one window and one segment length for both sorts: h can join the batch
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    expect = expected_launches(4, True, True, match, env)
    assert expect == (2 if env else 1)
    d = DistributedWitnessMap(prover._ctx.lib, prover._ctx.handle, prover._ck(gm).handle, 0, 1, "cuda:0")
    try:
        z_dev = torch.from_numpy(np.ascontiguousarray(ck.z).view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        for it in range(2):
            h = d.run(z_dev.data_ptr(), z_dev.shape[0], True, None)
            part = prover.prove_partial_h(gp, gm, ck.z, (0, 1), h.data_ptr(), d.M)
            assert prover.timings()["g1_pass_launches"] == expect, (it, prover.timings()["g1_pass_launches"], expect)
            proof = prover.prove_finalize(gp, ck.num_inputs, [part], world["r"], world["s"], (0, 1), dist_h=True)
            assert (proof.flat() == cs["want"]).all(), "proof %d differs from the oracle's" % it
        torch.cuda.synchronize()
        assert (h.cpu().numpy().view(np.uint64) == cs["h"]).all()
    finally:
        d.close()
