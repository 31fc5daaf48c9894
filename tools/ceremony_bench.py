#!/usr/bin/env python3
"""Time check_srs on one device, stage by stage, beside the derivation it guards.

For the SRS of a domain of n = 2^k points (2n - 1 powers in G1, n elsewhere), made by srs_from_trapdoor, on one curve:

  check_srs                         by stream events (g16_ceremony_get_timings): upload, membership, the coefficient sort, the bucket
                                    passes (with the base conversion in front of them), the reductions; the pairings and the whole
                                    call by the wall clock.  Fresh coefficients from the operating system, as a caller would use.
  generate_parameters_from_srs      on the same SRS in the same process, for SYN(k), by the wall clock: the yardstick -- the check is
                                    reported as a share of it

The honest SRS must pass and one with its last tau_g1 point replaced must fail before anything is reported.  One size per
invocation, so that each runs in a fresh process under a time limit of its own, smallest first:

    python tools/ceremony_bench.py --curve bls12_381 --k 16 --out profiles/ceremony_mi355x.jsonl

--all runs k = 16, 18, 20, 22 for the curve, each in a child process of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (16, 18, 20, 22)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--all", action="store_true", help="k = 16, 18, 20, 22, one child process each")
    ap.add_argument("--limit", type=int, default=600, help="seconds a child of --all may take")
    ap.add_argument("--no-derive", action="store_true", help="skip generate_parameters_from_srs (the check alone)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.all:
        for k in SIZES:   # a fresh child per size; the first failure or overrun ends the series
            cmd = [sys.executable, os.path.abspath(__file__), "--curve", args.curve, "--k", str(k), "--device", str(args.device)]
            cmd += (["--out", args.out] if args.out else []) + (["--no-derive"] if args.no_derive else [])
            rc = subprocess.run(cmd, timeout=args.limit).returncode
            if rc != 0:
                sys.exit(f"k = {k} ended with status {rc}; nothing larger was started")
        return

    import torch

    if not torch.cuda.is_available():
        sys.exit("ceremony_bench.py needs a GPU: a check is timed on the device or not at all")
    import groth16_amd as g
    from groth16_amd.binding import CURVE_ID, ptr32, ptr64
    from groth16_amd.groth16 import _GENERATORS, _fq_mont, _rand_fr

    curve, k = args.curve, args.k
    n = 1 << k
    import random

    rng = random.Random(2024)
    tau, alpha, beta = (_rand_fr(curve, rng, nonzero=True) for _ in range(3))
    g1s, g2s = _GENERATORS[curve]
    g1 = _fq_mont(curve, list(g1s))
    g2 = _fq_mont(curve, [g2s[0][0], g2s[0][1], g2s[1][0], g2s[1][1]])
    prover = g.Groth16(curve, device=args.device)
    t0 = time.perf_counter()
    srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
    t1 = time.perf_counter()
    res = prover.check_srs(srs)                      # the first call: code loading and arena growth are inside the figure
    t2 = time.perf_counter()
    first = prover.ceremony_timings()
    res2 = prover.check_srs(srs)                     # the second: the arena is there, the code is loaded
    t3 = time.perf_counter()
    ev = prover.ceremony_timings()
    assert res and res2, f"the honest SRS fails: {res.failed} {res2.failed}"
    last = len(srs.tau_g1) - 1
    srs.tau_g1[last] = srs.tau_g1[last - 1]          # a subgroup point in the wrong place: only the last coefficient meets it
    bad = prover.check_srs(srs)
    assert bad.failed == ("TAU_G1",), f"the tampered SRS gives {bad.failed}"
    srs.tau_g1[last] = 0
    bad = prover.check_srs(srs)
    assert bad.failed == ("BAD_POINT",) and (bad.array, bad.index, bad.reason) == ("tau_g1", last, 4), (bad.failed, bad.array, bad.index)
    plan = g.rlc_plan(2 * n - 2)
    line = dict(tool="ceremony_bench", curve=curve, k=k, domain=n, points=dict(tau_g1=2 * n - 1, tau_g2=n, alpha_tau_g1=n, beta_tau_g1=n),
                window_bits=plan["window_bits"], windows=plan["windows"], cpus=len(os.sched_getaffinity(0)),
                device=torch.cuda.get_device_name(args.device), srs_from_trapdoor_s=round(t1 - t0, 4), check_first_wall_s=round(t2 - t1, 4),
                check_wall_s=round(t3 - t2, 4), first_call_ms={a: round(b, 3) for a, b in first.items()}, **{a: round(b, 3) for a, b in ev.items()})
    if not args.no_derive:
        srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
        lb = g.lib()
        nc = n - 2
        z = np.zeros((nc + 3, 4), dtype=np.uint64)
        row_ptr = np.zeros(nc + 1, dtype=np.uint64)
        cols = [np.zeros(nc, dtype=np.uint32) for _ in range(3)]
        val = np.zeros((nc, 4), dtype=np.uint64)
        lb.check(lb.c.g16_synth_circuit(CURVE_ID[curve], k, 7, ptr64(z.reshape(-1)), ptr64(row_ptr), ptr32(cols[0]), ptr32(cols[1]),
                                        ptr32(cols[2]), ptr64(val.reshape(-1))))
        mats = g.ConstraintMatrices(2, nc + 1, nc, *[(row_ptr, c, val) for c in cols])
        t4 = time.perf_counter()
        prover.generate_parameters_from_srs(mats, srs)
        t5 = time.perf_counter()
        line.update(from_srs_wall_s=round(t5 - t4, 4), check_share_of_derivation=round((t3 - t2) / (t5 - t4), 4))
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    prover.close()


if __name__ == "__main__":
    main()
