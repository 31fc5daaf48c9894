#!/usr/bin/env python3
"""Cost of the R1CS satisfaction check (g16_circuit_check, g16_prove_checked) on one MI355X.

    python tools/check_bench.py [--k 22] [--curves bls12_381 bn254] [--reps 5] [--out profiles/check_mi355x.jsonl]

Per curve, in ONE process, over SYN(k) (g16_synth_circuit: 2^k - 2 constraints, one unit term per row and matrix) with the circuit
and a key resident on the GPU (bench.py's DeviceProver; --key synthetic, the default, loads distinct points instead of a CRS: the
prover's work is the same), best of --reps calls after one warm-up call, host clock around the call (every call ends in a stream
synchronisation); `spread` is (slowest - fastest) / fastest of the timed calls:
  check_resident_ms   g16_circuit_check, the assignment already in HBM: the kernel, the 16-byte read-back, the launch overhead
  check_host_ms       g16_circuit_check from a host assignment: the same plus ONE upload of 32 * (2^k + 1) bytes from pageable memory
  prove_ms / prove_checked_ms            g16_prove / g16_prove_checked, resident assignment (the check in place)
  prove_host_ms / prove_checked_host_ms  the same from a host assignment: g16_prove uploads in pieces under its first mat-vec rows,
                                         g16_prove_checked uploads once, checks, and proves from the resident copy
Every checked proof is compared byte for byte with the unchecked one, and the check must answer "satisfied".  One JSON line per curve
is printed and appended to --out.  No figure here is asserted by a test."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from groth16_amd.binding import CheckResultC, ProofC, ptr64  # noqa: E402


def timed(call, reps):
    call()   # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    return min(ts), (max(ts) - min(ts)) / min(ts)


def one_curve(curve, k, reps, key):
    p = bench.DeviceProver(curve, k, 1, 0, 1, 0, key=key)
    lb, c = p.lib, p.lib.c
    res = CheckResultC()
    host, dev = C.c_void_p(p.z_host.ctypes.data), C.c_void_p(p.z_dev.data_ptr())

    def check(ptr, on_device):
        lb.check(c.g16_circuit_check(p.ctx, p.ck, ptr, p.nvars, on_device, C.byref(res)))
        assert res.n_unsatisfied == 0, "the benchmark's own witness fails the check"

    def prove(ptr, on_device, checked, out):
        if checked:
            lb.check(c.g16_prove_checked(p.ctx, p.pk, p.ck, ptr, p.nvars, on_device, ptr64(p.r), ptr64(p.s), C.byref(out), C.byref(res)), res)
        else:
            lb.check(c.g16_prove(p.ctx, p.pk, p.ck, ptr, p.nvars, on_device, ptr64(p.r), ptr64(p.s), C.byref(out)))

    proofs = [ProofC() for _ in range(4)]
    line = dict(curve=curve, k=k, constraints=p.nc, key=key, reps=reps)
    for name, call in (("check_resident", lambda: check(dev, 1)), ("check_host", lambda: check(host, 0)),
                       ("prove", lambda: prove(dev, 1, False, proofs[0])), ("prove_checked", lambda: prove(dev, 1, True, proofs[1])),
                       ("prove_host", lambda: prove(host, 0, False, proofs[2])), ("prove_checked_host", lambda: prove(host, 0, True, proofs[3]))):
        best, spread = timed(call, reps)
        line[name + "_ms"] = round(best * 1e3, 3)
        line[name + "_spread"] = round(spread, 4)
    assert bytes(proofs[0]) == bytes(proofs[1]) == bytes(proofs[2]) == bytes(proofs[3]), "a checked proof differs from the unchecked one"
    line["checked_minus_plain_ms"] = round(line["prove_checked_ms"] - line["prove_ms"], 3)
    line["checked_minus_plain_host_ms"] = round(line["prove_checked_host_ms"] - line["prove_host_ms"], 3)
    p.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=22)
    ap.add_argument("--curves", nargs="+", default=["bls12_381", "bn254"], choices=["bls12_381", "bn254"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--key", default="synthetic", choices=["synthetic", "valid"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_mi355x.jsonl"))
    a = ap.parse_args()
    for curve in a.curves:
        line = json.dumps(one_curve(curve, a.k, a.reps, a.key))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
