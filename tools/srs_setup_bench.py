#!/usr/bin/env python3
"""Time the setup from an SRS on one device, phase by phase, beside the only other setup this library has.

For SYN(k) -- the benchmark's synthetic circuit: 2^k - 2 constraints, a domain of 2^k points, every coefficient 1 -- on one curve:

  srs_from_trapdoor                 the SRS itself (test utility; wall clock, reported for completeness)
  generate_parameters_from_srs      by stream events (g16_srs_get_timings): the four group transforms, the sparse products, the h step;
                                    and the whole call by the wall clock (host transposition, uploads and downloads included)
  contribute_delta                  the delta step by stream events, the whole call by the wall clock
  generate_parameters_with_qap      the toxic-waste generator on the same matrices, same process, wall clock: the yardstick

The two keys are compared byte for byte before anything is reported.  One size per invocation, so that each runs under a time limit
of its own, smallest first:

    python tools/srs_setup_bench.py --curve bls12_381 --k 16 --out profiles/srs_setup_mi355x.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--qap", default="libsnark", choices=["libsnark", "circom"])
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("srs_setup_bench.py needs a GPU: a setup is timed on the device or not at all")
    import groth16_amd as g
    from groth16_amd.binding import CURVE_ID, ptr32, ptr64
    from groth16_amd.groth16 import _rand_fr

    curve, k = args.curve, args.k
    lb = g.lib()
    nc = (1 << k) - 2
    z = np.zeros((nc + 3, 4), dtype=np.uint64)
    row_ptr = np.zeros(nc + 1, dtype=np.uint64)
    cols = [np.zeros(nc, dtype=np.uint32) for _ in range(3)]
    val = np.zeros((nc, 4), dtype=np.uint64)
    lb.check(lb.c.g16_synth_circuit(CURVE_ID[curve], k, 7, ptr64(z.reshape(-1)), ptr64(row_ptr), ptr32(cols[0]), ptr32(cols[1]), ptr32(cols[2]),
                                    ptr64(val.reshape(-1))))
    mats = g.ConstraintMatrices(2, nc + 1, nc, *[(row_ptr, c, val) for c in cols])
    n = 1 << k

    import random

    rng = random.Random(2024)
    tau, alpha, beta, delta = (_rand_fr(curve, rng, nonzero=True) for _ in range(4))
    qap = g.LibsnarkReduction if args.qap == "libsnark" else g.CircomReduction
    prover = g.Groth16(curve, device=args.device, qap=qap)   # one context for every call

    # the curve's standard generators, and gamma = 1 (Montgomery form)
    from groth16_amd.groth16 import _GENERATORS, _MODULUS_R, _fq_mont, _limbs

    g1s, g2s = _GENERATORS[curve]
    g1 = _fq_mont(curve, list(g1s))
    g2 = _fq_mont(curve, [g2s[0][0], g2s[0][1], g2s[1][0], g2s[1][1]])
    fr_one = np.array(_limbs((1 << 256) % _MODULUS_R[curve], 4), dtype=np.uint64)

    best = None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
        t1 = time.perf_counter()
        base = prover.generate_parameters_from_srs(mats, srs)
        t2 = time.perf_counter()
        key = prover.contribute_delta(base, delta)
        t3 = time.perf_counter()
        ev = prover.srs_timings()
        want = prover.generate_parameters_with_qap(mats, alpha, beta, fr_one, delta, g1, g2, tau)
        t4 = time.perf_counter()
        for f in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2", "gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query",
                  "h_query", "l_query"):
            assert (getattr(key, f) == getattr(want, f)).all(), f"the SRS-derived key differs from the toxic-waste key in {f}"
        run = dict(srs_from_trapdoor_s=t1 - t0, from_srs_wall_s=t2 - t1, delta_wall_s=t3 - t2, toxic_waste_wall_s=t4 - t3,
                   transforms_ms=ev["transforms_ms"], products_ms=ev["products_ms"], h_ms=ev["h_ms"], delta_ms=ev["delta_ms"])
        if best is None or run["from_srs_wall_s"] < best["from_srs_wall_s"]:
            best = run
    line = dict(tool="srs_setup_bench", curve=curve, k=k, qap=args.qap, domain=n, reps=args.reps, segment_len=int(lb.c.g16_srs_segment_len()),
                cpus=len(os.sched_getaffinity(0)), device=torch.cuda.get_device_name(args.device), keys_equal=True,
                **{name: round(v, 4) for name, v in best.items()},
                from_srs_over_toxic_waste=round((best["from_srs_wall_s"] + best["delta_wall_s"]) / best["toxic_waste_wall_s"], 2))
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    prover.close()


if __name__ == "__main__":
    main()
