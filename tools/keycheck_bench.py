#!/usr/bin/env python3
"""Time the key check without the derivation on one device, beside the derivation-based check it replaces and beside check_srs.

For the benchmark's synthetic circuit SYN(k) (domain n = 2^k), an SRS made by srs_from_trapdoor and the key derived from it with one
delta contribution, on one curve, all three on the same inputs in one process:

  check_key_derivation              the wall clock of the whole call (host argument checks, uploads and pairings included) and the stages
                                    by stream events (g16_keycheck_get_timings), with the plan of the full-size scalar sorts
  check_parameters(derive=True)     the parent's way: check_srs + generate_parameters_from_srs + check_delta_contribution, wall clock
  check_srs                         wall clock

Every figure is the SECOND call of its kind in the process (for the derivation: the second generate_parameters_from_srs -- the first
one made the key under test), so code loading and arena growth are outside.  The honest key must pass all three and a key with one
a_query point replaced must fail both key checks before anything is reported.  One size per invocation, so that each runs in a fresh
process under a time limit of its own, smallest first:

    python tools/keycheck_bench.py --curve bls12_381 --k 16 --out profiles/keycheck_mi355x.jsonl

--all runs k = 16 .. 22 for the curve, each in a child process of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (16, 17, 18, 19, 20, 21, 22)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--all", action="store_true", help="k = 16 .. 22, one child process each")
    ap.add_argument("--limit", type=int, default=900, help="seconds a child of --all may take")
    ap.add_argument("--qap", default="libsnark", choices=["libsnark", "circom"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.all:
        for k in SIZES:   # a fresh child per size; the first failure or overrun ends the series
            cmd = [sys.executable, os.path.abspath(__file__), "--curve", args.curve, "--k", str(k), "--device", str(args.device), "--qap", args.qap]
            cmd += ["--out", args.out] if args.out else []
            rc = subprocess.run(cmd, timeout=args.limit).returncode
            if rc != 0:
                sys.exit(f"k = {k} ended with status {rc}; nothing larger was started")
        return

    import torch

    if not torch.cuda.is_available():
        sys.exit("keycheck_bench.py needs a GPU: a check is timed on the device or not at all")
    import random

    import groth16_amd as g
    from groth16_amd.binding import CURVE_ID, ptr32, ptr64
    from groth16_amd.groth16 import _GENERATORS, _fq_mont, _rand_fr

    curve, k = args.curve, args.k
    n = 1 << k
    rng = random.Random(2024)
    tau, alpha, beta, delta = (_rand_fr(curve, rng, nonzero=True) for _ in range(4))
    g1s, g2s = _GENERATORS[curve]
    g1 = _fq_mont(curve, list(g1s))
    g2 = _fq_mont(curve, [g2s[0][0], g2s[0][1], g2s[1][0], g2s[1][1]])
    prover = g.Groth16(curve, device=args.device, qap=g.LibsnarkReduction if args.qap == "libsnark" else g.CircomReduction)
    srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
    lb = g.lib()
    nc = n - 2
    z = np.zeros((nc + 3, 4), dtype=np.uint64)
    row_ptr = np.zeros(nc + 1, dtype=np.uint64)
    cols = [np.zeros(nc, dtype=np.uint32) for _ in range(3)]
    val = np.zeros((nc, 4), dtype=np.uint64)
    lb.check(lb.c.g16_synth_circuit(CURVE_ID[curve], k, 7, ptr64(z.reshape(-1)), ptr64(row_ptr), ptr32(cols[0]), ptr32(cols[1]), ptr32(cols[2]),
                                    ptr64(val.reshape(-1))))
    mats = g.ConstraintMatrices(2, nc + 1, nc, *[(row_ptr, c, val) for c in cols])
    t0 = time.perf_counter()
    key = prover.contribute_delta(prover.generate_parameters_from_srs(mats, srs), delta)      # the first derivation of the process
    t1 = time.perf_counter()

    def timed(fn):
        a = time.perf_counter()
        res = fn()
        return res, time.perf_counter() - a

    first, first_s = timed(lambda: prover.check_key_derivation(mats, srs, key))
    first_ev = prover.keycheck_timings()
    res, check_s = timed(lambda: prover.check_key_derivation(mats, srs, key))
    ev = prover.keycheck_timings()
    assert first and res, f"the honest key fails: {first.failed} {res.failed}"
    _, _ = timed(lambda: prover.check_srs(srs))
    srs_res, srs_s = timed(lambda: prover.check_srs(srs))
    assert srs_res, srs_res.failed
    old, old_s = timed(lambda: prover.check_parameters(mats, srs, key))                       # derives the key again: the second derivation
    assert old, f"the derivation-based check fails the honest key: {old.failed}"
    saved = key.a_query[n // 2].copy()
    key.a_query[n // 2] = key.a_query[n // 2 - 1]        # a subgroup point in the wrong place
    bad = prover.check_key_derivation(mats, srs, key)
    assert bad.failed == ("A",), f"the tampered key gives {bad.failed}"
    key.a_query[n // 2] = saved
    stages = {a: b for a, b in ev.items() if a.endswith("_ms")}
    line = dict(tool="keycheck_bench", curve=curve, qap=args.qap, k=k, domain=n, variables=nc + 3, cpus=len(os.sched_getaffinity(0)),
                device=torch.cuda.get_device_name(args.device), runs=1, setup_and_first_derivation_s=round(t1 - t0, 4),
                check_key_derivation_first_wall_s=round(first_s, 4), check_key_derivation_wall_s=round(check_s, 4),
                check_parameters_derive_wall_s=round(old_s, 4), check_srs_wall_s=round(srs_s, 4),
                speedup_over_derivation_based=round(old_s / check_s, 2), share_of_check_srs=round(check_s / srs_s, 2),
                plan=dict(bases="raw", window_bits=int(ev["window_bits"]), windows=int(ev["windows"])),
                dominant_stage=max(stages, key=stages.get), first_call_ms={a: round(b, 3) for a, b in first_ev.items() if a.endswith("_ms")},
                **{a: round(b, 3) for a, b in stages.items()})
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    prover.close()


if __name__ == "__main__":
    main()
