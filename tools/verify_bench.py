#!/usr/bin/env python3
"""Throughput of the GPU Groth16 verifier (g16_verify_batch) and of this library's host C++ verifier (g16_host_verify).

    python tools/verify_bench.py --curve bls12_381 --n 1024 [--reps 3]     one JSON line per call
    python tools/verify_bench.py --curve bn254 --host [--reps 20]
    python tools/verify_bench.py --curve bls12_381 --n 65536 --aggregate [--reps 5]
    python tools/verify_bench.py --curve bls12_381 --n 65536 --subgroup [--reps 5]
    python tools/verify_bench.py --curve bls12_381 --n 65536 --decompress [--reps 5] [--out profiles/decompress_mi355x.jsonl]
    python tools/verify_bench.py --curve bls12_381 --n 65536 --mixed 1 64 4096 [--reps 3] [--out profiles/verify_mixed_mi355x.jsonl]

--n: proofs per g16_verify_batch call (copies of rerandomised honest proofs of a small SYN circuit, one public input); the line
reports the g16_pvk_load time, the best of --reps timed calls after one warm-up call (host clock around the call, which ends in a
device synchronise; includes the host->device copy of the proofs), and proofs/s.  --host: single-thread proofs/s of
g16_host_verify -- this library's host C++ on the same pairing templates, NOT ark-groth16.  --aggregate: g16_verify_aggregate (one
randomised equation per batch, coefficients drawn by the library) on the same batch, clock and warm-up, and in the same process
g16_verify_batch for the same n; both get the public inputs as one (n, l, 4) array, so neither figure carries a Python loop over the
proofs.  --subgroup: on one batch and in one process g16_verify_aggregate, g16_verify_aggregate_checked,
g16_check_proof_subgroups alone, and the host path the last one replaces -- g16_deserialize_points(validate=2) over the same 3n
points (uncompressed bytes, so no square root is in the figure) on the CPUs the process may use; the line reports the ratios
checked / aggregate and host / GPU check.  --decompress: on one batch of compressed proofs and in one process (a)
g16_decompress_proofs, (b) the host's g16_deserialize_points(compressed, validate=0) over the same 3n points on the CPUs the process
may use, (c) g16_verify_aggregate_bytes, (d) g16_verify_aggregate_checked on the already decoded proofs -- the floor of (c) -- and
(e) the host path that (c) replaces: (b) followed by (d); --out appends the line to a file.  --mixed K ..: a stream of n proofs that interleaves K verifying keys (key_of[i] = i mod K; four prepared keys with their own
trapdoors listed in turn to reach K, which is the same work).  Per K, in one process: g16_verify_aggregate_mixed through the C ABI
(best of --reps after a warm-up), and what the library offered before it for the same batch, already split by key outside the
clock -- one g16_verify_aggregate per key, and one g16_verify_batch per key (each loop timed once after a warm-up call; at K = 4096
they take seconds to minutes) -- and g16_verify_aggregate on n proofs under ONE key as the K = 1 yardstick.  `speedup` is the
faster of the two loops over the mixed call; --out appends the lines to a file (default profiles/verify_mixed_mi355x.jsonl).
`spread` is (slowest - fastest) / fastest of the --reps timed calls.  Run each step under its own time limit."""
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
    ap.add_argument("--subgroup", action="store_true")
    ap.add_argument("--decompress", action="store_true")
    ap.add_argument("--mixed", type=int, nargs="+", metavar="K", help="numbers of keys to interleave in one batch")
    ap.add_argument("--out", help="append the JSON line of --decompress / the lines of --mixed to this file")
    a = ap.parse_args()
    if a.mixed:
        return mixed(a)
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
    if a.decompress:
        return decompress(a, vk, flat, np.ascontiguousarray(np.broadcast_to(x.reshape(1, -1, 4), (a.n,) + x.reshape(-1, 4).shape)), L)
    if a.subgroup:
        return subgroup(a, vk, flat, np.ascontiguousarray(np.broadcast_to(x.reshape(1, -1, 4), (a.n,) + x.reshape(-1, 4).shape)), L)
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


def subgroup(a, vk, flat, xs, L):
    from groth16_amd.serialize import deserialize_points, serialize_points
    g1 = np.ascontiguousarray(np.concatenate([flat[:, : 2 * L], flat[:, 6 * L:]]))
    g2 = np.ascontiguousarray(flat[:, 2 * L: 6 * L])
    b1, b2 = serialize_points(a.curve, g1, False, compressed=False), serialize_points(a.curve, g2, True, compressed=False)

    def host():
        deserialize_points(a.curve, b1, 2 * a.n, False, compressed=False, validate=2)
        deserialize_points(a.curve, b2, a.n, True, compressed=False, validate=2)

    with g.Groth16(a.curve, device=0) as prover:
        pvk = prover.prepare_verifying_key(vk)
        assert prover.verify_aggregate_verdict(pvk, flat, xs, check_subgroups=True) == 1, "the benchmark batch was rejected"
        assert (prover.check_proof_subgroups(flat) == 1).all()
        agg, agg_spread = timed(lambda: prover.verify_aggregate_verdict(pvk, flat, xs), a.reps)
        chk, chk_spread = timed(lambda: prover.verify_aggregate_verdict(pvk, flat, xs, check_subgroups=True), a.reps)
        sub, sub_spread = timed(lambda: prover.check_proof_subgroups(flat), a.reps)
        pvk.close()
    hst, hst_spread = timed(host, a.reps)
    print(json.dumps(dict(curve=a.curve, n=a.n, mode="subgroup", aggregate_ms=round(agg * 1e3, 3), aggregate_spread=round(agg_spread, 4),
                          checked_ms=round(chk * 1e3, 3), checked_spread=round(chk_spread, 4), check_only_ms=round(sub * 1e3, 3),
                          check_only_spread=round(sub_spread, 4), host_validate_ms=round(hst * 1e3, 3), host_spread=round(hst_spread, 4),
                          checked_over_aggregate=round(chk / agg, 3), host_over_gpu_check=round(hst / sub, 1), reps=a.reps)))


def decompress(a, vk, flat, xs, L):
    from groth16_amd.serialize import deserialize_points, serialize_points
    fb = 48 if a.curve == "bls12_381" else 32
    data = np.zeros((a.n, 4 * fb), dtype=np.uint8)   # n x (A | B | C), the layout of proof_to_bytes(compressed=True)
    for lo, hi, g2, at, size in ((0, 2 * L, False, 0, fb), (2 * L, 6 * L, True, fb, 2 * fb), (6 * L, 8 * L, False, 3 * fb, fb)):
        data[:, at: at + size] = np.frombuffer(serialize_points(a.curve, np.ascontiguousarray(flat[:, lo:hi]), g2), dtype=np.uint8).reshape(a.n, size)
    b1 = np.ascontiguousarray(np.concatenate([data[:, :fb], data[:, 3 * fb:]])).tobytes()
    b2 = np.ascontiguousarray(data[:, fb: 3 * fb]).tobytes()

    def host_decode():
        deserialize_points(a.curve, b1, 2 * a.n, False, compressed=True, validate=0)
        deserialize_points(a.curve, b2, a.n, True, compressed=True, validate=0)

    with g.Groth16(a.curve, device=0) as prover:
        pvk = prover.prepare_verifying_key(vk)
        decoded, status = prover.decompress_proofs(data)
        assert (status == 1).all() and decoded.tobytes() == flat.tobytes(), "the GPU decoded the benchmark batch differently"
        assert prover.verify_aggregate_bytes_verdict(pvk, data, xs) == 1, "the benchmark batch was rejected"
        dec, dec_spread = timed(lambda: prover.decompress_proofs(data), a.reps)
        hst, hst_spread = timed(host_decode, a.reps)
        fused, fused_spread = timed(lambda: prover.verify_aggregate_bytes_verdict(pvk, data, xs), a.reps)
        chk, chk_spread = timed(lambda: prover.verify_aggregate_verdict(pvk, flat, xs, check_subgroups=True), a.reps)

        def host_path():
            host_decode()
            prover.verify_aggregate_verdict(pvk, flat, xs, check_subgroups=True)

        path, path_spread = timed(host_path, a.reps)
        pvk.close()
    line = json.dumps(dict(curve=a.curve, n=a.n, mode="decompress", cpus=len(os.sched_getaffinity(0)),
                           gpu_decompress_ms=round(dec * 1e3, 3), gpu_decompress_spread=round(dec_spread, 4),
                           gpu_decompress_proofs_per_s=round(a.n / dec, 1),
                           host_decompress_ms=round(hst * 1e3, 3), host_decompress_spread=round(hst_spread, 4),
                           host_decompress_proofs_per_s=round(a.n / hst, 1),
                           bytes_to_verdict_ms=round(fused * 1e3, 3), bytes_to_verdict_spread=round(fused_spread, 4),
                           bytes_to_verdict_proofs_per_s=round(a.n / fused, 1),
                           checked_decoded_ms=round(chk * 1e3, 3), checked_decoded_spread=round(chk_spread, 4),
                           host_decode_then_checked_ms=round(path * 1e3, 3), host_decode_then_checked_spread=round(path_spread, 4),
                           host_over_gpu_decompress=round(hst / dec, 1), bytes_over_checked=round(fused / chk, 3),
                           host_path_over_bytes=round(path / fused, 2), reps=a.reps))
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def mixed(a):
    import ctypes as C

    from groth16_amd.binding import lib, ptr32, ptr64
    from mixed_key_cases import mixed_keys
    cases = [mixed_keys(a.curve, 8)[k] for k in (0, 1, 2, 7)]   # three set-ups and a derived key, the same input count
    n = a.n
    out = a.out or os.path.join(ROOT, "profiles", "verify_mixed_mi355x.jsonl")
    lb = lib()
    with g.Groth16(a.curve, device=0) as prover:
        prepared = [prover.prepare_verifying_key(c.vk) for c in cases]
        single = np.ascontiguousarray(np.stack([cases[0].proofs[i % 2] for i in range(n)]))
        single_x = np.ascontiguousarray(np.broadcast_to(cases[0].vectors[0].reshape(1, -1, 4), (n,) + cases[0].vectors[0].reshape(-1, 4).shape))
        assert prover.verify_aggregate_verdict(prepared[0], single, single_x) == 1
        one_key, one_key_spread = timed(lambda: prover.verify_aggregate_verdict(prepared[0], single, single_x), a.reps)
        for K in a.mixed:
            assert 1 <= K <= n
            key_of = (np.arange(n) % K).astype(np.uint32)
            which = key_of % len(cases)
            flat = np.ascontiguousarray(np.stack([cases[w].proofs[(i // K) % 2] for i, w in enumerate(which)]))
            x = np.ascontiguousarray(np.stack([cases[w].vectors[0].reshape(-1, 4) for w in which]))   # (n, l, 4): equal counts here
            handles = (C.c_void_p * K)(*[prepared[k % len(cases)].handle for k in range(K)])
            v = np.zeros(1, dtype=np.uint8)

            def call():
                lb.check(lb.c.g16_verify_aggregate_mixed(prover._ctx.handle, handles, K, ptr32(key_of), ptr64(flat.reshape(-1)), n, ptr64(x.reshape(-1)),
                                                         x.size // 4, None, 0, v.ctypes.data_as(C.c_void_p)))
                assert v[0] == 1, "the benchmark batch was rejected"

            mix, mix_spread = timed(call, a.reps)
            parts = [(prepared[k % len(cases)], np.ascontiguousarray(flat[k::K]), np.ascontiguousarray(x[k::K])) for k in range(K)]

            def loop(fn):
                fn(*parts[0])   # warm-up
                t = time.perf_counter()
                for done, part in enumerate(parts):
                    fn(*part)
                    if done % 512 == 511:
                        print(f"  K = {K}: {done + 1} per-key calls", file=sys.stderr, flush=True)
                return time.perf_counter() - t

            def agg_one(pvk, fl, xs):
                assert prover.verify_aggregate_verdict(pvk, fl, xs) == 1

            def batch_one(pvk, fl, xs):
                assert (prover.verify_verdicts(pvk, fl, xs) == 1).all()

            agg_loop, batch_loop = loop(agg_one), loop(batch_one)
            best = min(agg_loop, batch_loop)
            line = json.dumps(dict(curve=a.curve, n=n, mode="mixed", keys=K, distinct_keys=min(K, len(cases)),
                                   mixed_ms=round(mix * 1e3, 3), mixed_spread=round(mix_spread, 4), mixed_proofs_per_s=round(n / mix, 1),
                                   per_key_aggregate_loop_ms=round(agg_loop * 1e3, 3), per_key_batch_loop_ms=round(batch_loop * 1e3, 3),
                                   speedup=round(best / mix, 3), one_key_aggregate_ms=round(one_key * 1e3, 3),
                                   one_key_aggregate_spread=round(one_key_spread, 4), mixed_over_one_key_aggregate=round(mix / one_key, 3),
                                   reps=a.reps))
            print(line, flush=True)
            with open(out, "a") as f:
                f.write(line + "\n")
        for p in prepared:
            p.close()


if __name__ == "__main__":
    main()
