#!/usr/bin/env python3
"""Throughput of the GPU Groth16 verifier (g16_verify_batch) and of this library's host C++ verifier (g16_host_verify).

    python tools/verify_bench.py --curve bls12_381 --n 1024 [--reps 3]     one JSON line per call
    python tools/verify_bench.py --curve bn254 --host [--reps 20]
    python tools/verify_bench.py --curve bls12_381 --n 65536 --aggregate [--reps 5]

--n: proofs per g16_verify_batch call (copies of rerandomised honest proofs of a small SYN circuit, one public input); the line
reports the g16_pvk_load time, the best of --reps timed calls after one warm-up call (host clock around the call, which ends in a
device synchronise; includes the host->device copy of the proofs), and proofs/s.  --host: single-thread proofs/s of
g16_host_verify -- this library's host C++ on the same pairing templates, NOT ark-groth16.  --aggregate: g16_verify_aggregate (one
randomised equation per batch, coefficients drawn by the library) on the same batch, clock and warm-up, and in the same process
g16_verify_batch for the same n; both get the public inputs as one (n, l, 4) array, so neither figure carries a Python loop over the
proofs.  `spread` is (slowest - fastest) / fastest of the --reps timed calls.  Run each step under its own time limit."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402

import groth16_amd as g  # noqa: E402
from verify_cases import oracle_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--aggregate", action="store_true")
    a = ap.parse_args()
    vk, proofs, x, cp = oracle_case(a.curve)
    L = cp.fq_limbs64
    if a.host:
        assert g.verify_proof_host(a.curve, vk, proofs[0], x)
        t = time.perf_counter()
        for _ in range(a.reps):
            g.verify_proof_host(a.curve, vk, proofs[0], x)
        dt = (time.perf_counter() - t) / a.reps
        print(json.dumps(dict(curve=a.curve, what="g16_host_verify (this library's host C++, one thread; not ark-groth16)",
                              ms_per_proof=round(dt * 1e3, 3), proofs_per_s=round(1 / dt, 1))))
        return
    base = [proofs[0]] + [g.rerandomize_proof(a.curve, vk, g.Proof(proofs[0][:2 * L], proofs[0][2 * L:6 * L], proofs[0][6 * L:])).flat()
                          for _ in range(7)]
    flat = np.ascontiguousarray(np.stack([base[i % len(base)] for i in range(a.n)]))
    xs = [x] * a.n
    if a.aggregate:
        return aggregate(a, vk, flat, np.ascontiguousarray(np.broadcast_to(x.reshape(1, -1, 4), (a.n,) + x.reshape(-1, 4).shape)))
    with g.Groth16(a.curve, device=0) as prover:
        t = time.perf_counter()
        pvk = prover.prepare_verifying_key(vk)
        load_ms = (time.perf_counter() - t) * 1e3
        ok = prover.verify_verdicts(pvk, flat, xs)   # warm-up, and every verdict must be 1
        assert (ok == 1).all(), "a proof of the benchmark batch was rejected"
        best = float("inf")
        for _ in range(a.reps):
            t = time.perf_counter()
            prover.verify_verdicts(pvk, flat, xs)
            best = min(best, time.perf_counter() - t)
        pvk.close()
    print(json.dumps(dict(curve=a.curve, n=a.n, pvk_load_ms=round(load_ms, 2), batch_ms=round(best * 1e3, 3),
                          proofs_per_s=round(a.n / best, 1), reps=a.reps)))


def timed(call, reps):
    call()   # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    return min(ts), (max(ts) - min(ts)) / min(ts)


def aggregate(a, vk, flat, xs):
    with g.Groth16(a.curve, device=0) as prover:
        pvk = prover.prepare_verifying_key(vk)
        assert prover.verify_aggregate_verdict(pvk, flat, xs) == 1, "the benchmark batch was rejected"
        assert (prover.verify_verdicts(pvk, flat, xs) == 1).all(), "a proof of the benchmark batch was rejected"
        agg, agg_spread = timed(lambda: prover.verify_aggregate_verdict(pvk, flat, xs), a.reps)
        each, each_spread = timed(lambda: prover.verify_verdicts(pvk, flat, xs), a.reps)
        pvk.close()
    print(json.dumps(dict(curve=a.curve, n=a.n, mode="aggregate", batch_ms=round(agg * 1e3, 3), proofs_per_s=round(a.n / agg, 1),
                          spread=round(agg_spread, 4), per_proof_batch_ms=round(each * 1e3, 3), per_proof_proofs_per_s=round(a.n / each, 1),
                          per_proof_spread=round(each_spread, 4), speedup=round(each / agg, 3), reps=a.reps)))


if __name__ == "__main__":
    main()
