"""The transforms and the witness map at the edge of their lazy ranges and at every pass plan, bit for bit against the CPU oracle
(run on the MI355X with -m gpu).  Equality with the oracle's canonical output is also the check that every stored element is
below p.

What the kernels of csrc/ntt.hip rely on and which case drives it to its ceiling is tabulated in DESIGN.md 4.2; the vectors
and the circuit that transforms three arbitrary vectors come from transform_cases.py, whose references test_transform_cases.py
pins to the big-int model on this very data.

  * test_ntt_every_size: g16_ntt (DIF passes + bit-reversal / scale) on random data at EVERY log n in 0..19 -- one pass up to
    10, two from 11, three from 19 (10 + 5 + 4, the first uneven split), lone radix-2 rounds at odd stage counts.
  * test_ntt_named_vectors: every named vector, all four modes, at the sizes around the plan changes.
  * test_witness_map_free_vectors: the fused DIF/DIT kernel, the pre-scaled DIT load, the fused quotient load and the
    three-chains-per-launch batches on arbitrary vectors (no satisfied system needed), both branches of the mat-vec.
  * test_distributed_map_free_vectors: ntt_dit_batch / ntt_dif_batch / dwm_column_kernel through the four stages on simulated
    ranks, against the oracle and the single-GPU map.

Cost of the references (oracle, 16 threads, measured on a CPU-only machine; BLS12-381 / BN254): one transform 0.04 / 0.02 s at
2^16, 0.19 / 0.06 s at 2^18, 0.11 / 0.11 s at 2^19; one witness map 0.32 / 0.12 s at k = 16, 1.26 / 0.45 s at k = 18,
1.00 / 0.82 s at k = 19.  Building a k = 19 triple costs 0.4 s per random vector, 0.65 s per geometric one and about 1.5 s for the
product of the satisfied triple.  The full list of triples at k = 19 would be 10 - 15 s of oracle and set-up per curve, so k = 19 runs the four
triples of transform_cases.TRIPLES_AT_19 (rand, pm1_all, geometric, satisfied), one per test, and the full list runs at 3, 10 and
11; the named vectors of a size are split over three tests (twenty oracle transforms each, 2.4 s at 2^19).  On an MI355X the whole
file (136 tests) takes 30 s; the slowest calls are the named vectors at 2^19 (1.3 - 1.7 s), the k = 19 maps (0.4 - 1.2 s) and
the distributed map at (16, 8) (0.9 s)."""
import numpy as np
import pytest

import transform_cases as tc
from test_gpu_dist_wm import mats_of, run_all_ranks

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
WM_SIZES = [1, 2, 3, 4, 6, 8, 10, 11, 12, 14, 15, 17, 19]
WM_ALL_TRIPLES = [3, 10, 11]      # + k = 19 with transform_cases.TRIPLES_AT_19 (the oracle's time, see above)
WM_BOTH_COEFFS = [3, 11]


@pytest.fixture(scope="module")
def g():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import groth16_amd

    return groth16_amd


@pytest.fixture(scope="module", params=CURVES)
def env(request, g, orc):
    prover = g.Groth16(request.param, 0)
    yield tc.CURVES[request.param], prover
    prover.close()


def check_ntt(prover, orc, cp, x, what):
    for inverse, coset in tc.MODES:
        got = prover.ntt(x, inverse, coset)
        want = orc.ntt(cp.name, x, inverse, coset)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "%s inverse=%s coset=%s: %d of %d elements differ, first at %d" % (what, inverse, coset, bad.size, len(x),
                                                                                               bad[0])


@pytest.mark.parametrize("log_n", list(range(20)))
def test_ntt_every_size(env, orc, log_n):
    cp, prover = env
    check_ntt(prover, orc, cp, orc.rand_fr(cp.name, 300 + log_n, 1 << log_n), "rand 2^%d" % log_n)


@pytest.mark.parametrize("log_n", [1, 2, 3, 9, 10, 11, 12, 18, 19])
@pytest.mark.parametrize("group", [0, 1, 2])
def test_ntt_named_vectors(env, orc, log_n, group):
    """(the names in three groups per size: at 2^19 a test is then twenty oracle transforms)"""
    cp, prover = env
    for name in tc.NAMES[group::3]:
        x = tc.vector_mont(cp, name, 1 << log_n, 400 + log_n, None, orc)
        check_ntt(prover, orc, cp, x, "%s 2^%d" % (name, log_n))


def check_wm(g, prover, orc, cp, k, tname, coeff, gms):
    va, vb, vc = tc.triple_mont(cp, k, tname, orc)
    ck = tc.free_vector_circuit(cp.name, k, va, vb, vc, coeff)
    if coeff not in gms:   # one device copy of the matrices per (k, coeff): the triples differ in z only
        gms[coeff] = mats_of(g, ck)
    gm = gms[coeff]
    h = prover.witness_map_from_matrices(gm, ck.num_inputs, ck.num_constraints, ck.z)
    want = orc.witness_map(ck)
    bad = np.flatnonzero((h != want).any(axis=1))
    assert bad.size == 0, "k=%d %s coeff=%s: %d of %d coefficients differ, first at %d" % (k, tname, "1" if coeff == 1 else "p-1",
                                                                                          bad.size, len(h), bad[0])
    if tname == "satisfied" and coeff == 1:
        assert not h[-1].any()   # deg h <= n - 2 for a satisfied system
    return ck, gm, want


@pytest.mark.parametrize("tname", tc.TRIPLES_AT_19)
def test_witness_map_free_vectors_three_passes(env, orc, g, tname):
    """k = 19: the smallest three-pass plan, 10 + 5 + 4 (one triple per test: the oracle's map is a second each)"""
    cp, prover = env
    try:
        check_wm(g, prover, orc, cp, 19, tname, 1, {})
    finally:
        prover.evict()


@pytest.mark.parametrize("k", [k for k in WM_SIZES if k != 19])
def test_witness_map_free_vectors(env, orc, g, k):
    cp, prover = env
    triples = list(tc.TRIPLES) if k in WM_ALL_TRIPLES else ["rand", "pm1_all"]
    gms = {}
    try:
        for coeff in (1, cp.r - 1) if k in WM_BOTH_COEFFS else (1,):
            for tname in triples:
                check_wm(g, prover, orc, cp, k, tname, coeff, gms)
    finally:
        prover.evict()


@pytest.mark.parametrize("k,world", [(6, 8), (10, 2), (10, 4), (12, 16), (16, 8)])
def test_distributed_map_free_vectors(env, orc, g, k, world):
    cp, prover = env
    gms = {}
    try:
        for tname in tc.TRIPLES:
            ck, gm, want = check_wm(g, prover, orc, cp, k, tname, 1, gms)   # the single-GPU map == oracle
            ranks, h = run_all_ranks(g, prover, gm, ck.z, world)
            for d in ranks:
                d.close()
            bad = np.flatnonzero((h != want).any(axis=1))
            assert bad.size == 0, "k=%d world=%d %s: %d of %d coefficients differ, first at %d" % (k, world, tname, bad.size, len(h), bad[0])
    finally:
        prover.evict()
