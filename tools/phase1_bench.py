#!/usr/bin/env python3
"""Time a phase-1 contribution on one device, stage by stage, beside the parent's uniform-scalar kernel.

For a domain of 2^k points on one curve, in ONE process:

  srs_from_trapdoor     the SRS itself (test utility; wall clock, reported for completeness): 2^(k+1) - 1 points of tau_g1, 2^k elsewhere
  contribute_tau        twice; the SECOND call is reported -- the whole call by the wall clock (copies of the arrays, uploads and downloads
                        included) and the stages by stream events (g16_phase1_get_timings).  mul_g1_pts_per_s = the G1 points of the three
                        G1 arrays over mul_g1_ms: the new kernel, a different scalar in every lane
  contribute_delta      on a key whose h_query is the 2^k points of alpha_tau_g1 (no l_query): srs_scale_kernel, ONE scalar for the whole
                        launch, by its stream events (g16_srs_get_timings) -- the bar.  scale_g1_pts_per_s beside it, and the ratio.

The contributed SRS is held against the contribution check before anything is reported.  One size per invocation, so that each runs in
a fresh process under a time limit of its own, smallest first:

    python tools/phase1_bench.py --curve bls12_381 --k 16 --out profiles/phase1_mi355x.jsonl

--host-rate N times the host twin (plain double-and-add, no GPU) on N G1 points spread over --workers processes (default 16)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _host_chunk(args):
    curve, seed, n = args
    import random

    import groth16_amd as g
    from groth16_amd.groth16 import _GENERATORS, _fq_mont, _rand_fr

    rng = random.Random(seed)
    gen = _fq_mont(curve, list(_GENERATORS[curve][0]))
    ks = np.array([_rand_fr(curve, rng, nonzero=True) for _ in range(n)], dtype=np.uint64)
    pts = g.batch_scalar_mul_host(curve, np.tile(gen, (n, 1)), ks)   # n distinct points (untimed)
    t0 = time.perf_counter()
    g.batch_scalar_mul_host(curve, pts, ks)
    return time.perf_counter() - t0


def host_rate(curve, n, out, workers):
    from concurrent.futures import ProcessPoolExecutor

    cpus = min(len(os.sched_getaffinity(0)), workers)
    per = (n + cpus - 1) // cpus
    jobs = [(curve, 100 + i, min(per, n - i * per)) for i in range(cpus) if i * per < n]
    t0 = time.perf_counter()
    with ProcessPoolExecutor(len(jobs)) as ex:
        inner = list(ex.map(_host_chunk, jobs))
    wall = time.perf_counter() - t0
    line = dict(tool="phase1_bench", mode="host_twin", curve=curve, points=n, cpus=cpus, slowest_worker_s=round(max(inner), 4),
                g1_pts_per_s=round(n / max(inner), 1), wall_with_startup_s=round(wall, 3))
    emit(line, out)


def emit(line, out):
    text = json.dumps(line)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-rate", type=int, default=0, metavar="N")
    ap.add_argument("--workers", type=int, default=16, help="processes of --host-rate (at most the CPUs the process may use)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.host_rate:
        return host_rate(args.curve, args.host_rate, args.out, args.workers)

    import torch

    if not torch.cuda.is_available():
        sys.exit("phase1_bench.py needs a GPU: a contribution is timed on the device or not at all")
    import random

    import groth16_amd as g
    from groth16_amd.groth16 import _GENERATORS, _fq_mont, _rand_fr

    curve, k = args.curve, args.k
    n = 1 << k
    rng = random.Random(2025)
    tau, alpha, beta, delta = (_rand_fr(curve, rng, nonzero=True) for _ in range(4))
    mine = [_rand_fr(curve, rng, nonzero=True) for _ in range(3)]
    g1s, g2s = _GENERATORS[curve]
    g1 = _fq_mont(curve, list(g1s))
    g2 = _fq_mont(curve, [g2s[0][0], g2s[0][1], g2s[1][0], g2s[1][1]])
    prover = g.Groth16(curve, device=args.device)   # one context for every call

    t0 = time.perf_counter()
    srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
    t_srs = time.perf_counter() - t0
    prover.contribute_tau(srs, *mine)              # the first call pays for the arena and the code object
    t0 = time.perf_counter()
    after, pub = prover.contribute_tau(srs, *mine)
    wall = time.perf_counter() - t0
    ev = prover.phase1_timings()
    t0 = time.perf_counter()
    res = prover.check_tau_contribution(srs, after, pub)
    t_check = time.perf_counter() - t0
    assert res.ok, res
    g1_points = (len(srs.tau_g1) - 1) + len(srs.alpha_tau_g1) + len(srs.beta_tau_g1)
    g2_points = len(srs.tau_g2) - 1

    # the bar: one scalar for every lane, the generic arithmetic (g16_params_apply_delta on n points of G1)
    z1 = np.zeros((0, srs.tau_g1.shape[1]), dtype=np.uint64)
    z2 = np.zeros((0, srs.tau_g2.shape[1]), dtype=np.uint64)
    key = g.ProvingKey(curve, srs.tau_g1[:1], srs.tau_g1[:1], srs.tau_g1[:1].copy(), srs.tau_g2[:1], srs.tau_g2[:1].copy(), z1, z1, z2,
                       np.ascontiguousarray(srs.alpha_tau_g1), z1, srs.tau_g2[:1], z1)
    prover.contribute_delta(key, delta)
    prover.contribute_delta(key, delta)
    delta_ms = prover.srs_timings()["delta_ms"]
    new_rate = g1_points / (ev["mul_g1_ms"] * 1e-3)
    old_rate = n / (delta_ms * 1e-3)
    line = dict(tool="phase1_bench", mode="contribute_tau", curve=curve, k=k, domain=n, g1_points=g1_points, g2_points=g2_points,
                chunk=int(os.environ.get("G16_PHASE1_CHUNK", 1 << 17)), cpus=len(os.sched_getaffinity(0)),
                device=torch.cuda.get_device_name(args.device), check_ok=True, srs_from_trapdoor_s=round(t_srs, 3),
                contribute_wall_s=round(wall, 4), check_wall_s=round(t_check, 3), **{name: round(v, 3) for name, v in ev.items()},
                mul_g1_pts_per_s=round(new_rate, 1), mul_g2_pts_per_s=round(g2_points / (ev["mul_g2_ms"] * 1e-3), 1),
                scale_points=n, scale_delta_ms=round(delta_ms, 3), scale_g1_pts_per_s=round(old_rate, 1),
                per_point_over_uniform_scalar=round(new_rate / old_rate, 3))
    emit(line, args.out)
    prover.close()


if __name__ == "__main__":
    main()
