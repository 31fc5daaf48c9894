#!/usr/bin/env python3
"""g16_witness_map over one synthetic circuit (g16_synth_circuit) loaded for both reductions, resident assignment, one process:
best of --reps calls after a warm-up per (curve, reduction), with the spread.  Two clocks per call, side by side:

  map_ms    g16_timings.witness_map_ms of that call: HIP events around the map alone (row kernel, transforms, pointwise kernel).
            THIS is the figure the two reductions are compared by; ntt_ms (the transforms inside it) goes with it.
  call_ms   host clock around the C entry point as a caller sees it: the map plus the download of its domain_size Fr of output
            into pageable host memory -- the same bytes for both reductions, and at 2^22 (128 MiB) the larger part of the call.

    python tools/circom_map_bench.py --k 22 --out profiles/circom_map_mi355x.jsonl

--curve / --qap restrict the run to one curve / one reduction (a kernel trace of one map alone)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return dict(best=round(min(xs), 3), worst=round(max(xs), 3), spread=round(max(xs) - min(xs), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--curve", choices=["bls12_381", "bn254"], default=None)
    ap.add_argument("--qap", choices=["libsnark", "circom"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import groth16_amd as g
    from groth16_amd.binding import CURVE_ID, lib, ptr32, ptr64

    lb = lib()
    k, nc = args.k, (1 << args.k) - 2
    qaps = [q for name, q in (("libsnark", g.LibsnarkReduction), ("circom", g.CircomReduction)) if args.qap in (None, name)]
    lines = []
    for curve in ([args.curve] if args.curve else ["bls12_381", "bn254"]):
        z = np.zeros((nc + 3, 4), dtype=np.uint64)
        row_ptr = np.zeros(nc + 1, dtype=np.uint64)
        cols = [np.zeros(nc, dtype=np.uint32) for _ in range(3)]
        val = np.zeros((nc, 4), dtype=np.uint64)
        lb.check(lb.c.g16_synth_circuit(CURVE_ID[curve], k, 7, ptr64(z), ptr64(row_ptr), ptr32(cols[0]), ptr32(cols[1]), ptr32(cols[2]), ptr64(val)))
        mats = g.ConstraintMatrices(2, nc + 1, nc, *[(row_ptr, c, val) for c in cols])
        z_dev = torch.from_numpy(z.view(np.int64)).cuda()
        h = np.zeros((1 << k, 4), dtype=np.uint64)
        for qap in qaps:
            with g.Groth16(curve, 0, qap=qap) as prover:
                dck = prover._ck(mats)
                call_ms, map_ms, ntt_ms = [], [], []
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lb.check(lb.c.g16_witness_map(prover._ctx.handle, dck.handle, C.c_void_p(z_dev.data_ptr()), nc + 3, 1, ptr64(h)))
                    t1 = time.perf_counter()
                    if rep:
                        tm = prover.timings()
                        call_ms.append((t1 - t0) * 1e3)
                        map_ms.append(tm["witness_map_ms"])
                        ntt_ms.append(tm["ntt_ms"])
            lines.append(dict(curve=curve, k=k, qap=qap.__name__, reps=args.reps, map_ms=spread(map_ms), ntt_ms=spread(ntt_ms),
                              call_ms=spread(call_ms), download_mib=h.nbytes / 2**20,
                              clocks="map_ms, ntt_ms: HIP events around the map alone (g16_timings of the call); call_ms: host clock around "
                                     "g16_witness_map, resident assignment, h downloaded to pageable memory"))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
