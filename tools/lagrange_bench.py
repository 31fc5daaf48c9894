#!/usr/bin/env python3
"""Time the Lagrange form of an SRS on one device beside the transforms of the existing derivation, and the key from it beside the
existing derivation as a whole.

For SYN(k) -- the benchmark's synthetic circuit: 2^k - 2 constraints, a domain of 2^k points -- on one curve, in ONE process:

  srs_from_trapdoor                   the SRS itself (test utility; wall clock, reported for completeness)
  prepare_srs                         twice; the SECOND call is reported -- the whole call by the wall clock and the four arrays and the
                                      h basis by stream events (g16_lagrange_get_timings; uploads and downloads included)
  generate_parameters_from_srs        the existing derivation on the same SRS: its transforms phase by stream events (g16_srs_get_timings)
                                      -- the code this change leaves as it was, so the bar is the parent's -- and the whole call by the
                                      wall clock
  generate_parameters_from_lagrange   twice; the SECOND call by the wall clock, its products by stream events

The two keys are compared byte for byte before anything is reported.  One size per invocation, so that each runs in a fresh process
under a time limit of its own, smallest first:

    python tools/lagrange_bench.py --curve bls12_381 --k 16 --out profiles/lagrange_mi355x.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEY_FIELDS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2", "gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query",
              "h_query", "l_query")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--qap", default="libsnark", choices=["libsnark", "circom"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("lagrange_bench.py needs a GPU: the transforms are timed on the device or not at all")
    import random

    import groth16_amd as g
    from groth16_amd.binding import CURVE_ID, ptr32, ptr64
    from groth16_amd.groth16 import _GENERATORS, _fq_mont, _rand_fr

    curve, k = args.curve, args.k
    lb = g.lib()
    n, nc = 1 << k, (1 << k) - 2
    z = np.zeros((nc + 3, 4), dtype=np.uint64)
    row_ptr = np.zeros(nc + 1, dtype=np.uint64)
    cols = [np.zeros(nc, dtype=np.uint32) for _ in range(3)]
    val = np.zeros((nc, 4), dtype=np.uint64)
    lb.check(lb.c.g16_synth_circuit(CURVE_ID[curve], k, 7, ptr64(z.reshape(-1)), ptr64(row_ptr), ptr32(cols[0]), ptr32(cols[1]), ptr32(cols[2]),
                                    ptr64(val.reshape(-1))))
    mats = g.ConstraintMatrices(2, nc + 1, nc, *[(row_ptr, c, val) for c in cols])
    rng = random.Random(2026)
    tau, alpha, beta = (_rand_fr(curve, rng, nonzero=True) for _ in range(3))
    g1s, g2s = _GENERATORS[curve]
    g1 = _fq_mont(curve, list(g1s))
    g2 = _fq_mont(curve, [g2s[0][0], g2s[0][1], g2s[1][0], g2s[1][1]])
    qap = g.LibsnarkReduction if args.qap == "libsnark" else g.CircomReduction
    prover = g.Groth16(curve, device=args.device, qap=qap)   # one context for every call

    t0 = time.perf_counter()
    srs = prover.srs_from_trapdoor(n, tau, alpha, beta, g1, g2)
    t_srs = time.perf_counter() - t0

    prover.prepare_srs(srs, log_n=k)               # the first call pays for the arena and the code object
    t0 = time.perf_counter()
    lag = prover.prepare_srs(srs, log_n=k)
    prepare_wall = time.perf_counter() - t0
    ev = prover.lagrange_timings()
    new_transforms_ms = ev["u_g1_ms"] + ev["alpha_u_g1_ms"] + ev["beta_u_g1_ms"] + ev["u_g2_ms"]

    t0 = time.perf_counter()
    want = prover.generate_parameters_from_srs(mats, srs)
    from_srs_wall = time.perf_counter() - t0
    old = prover.srs_timings()

    prover.generate_parameters_from_lagrange(mats, lag)
    t0 = time.perf_counter()
    got = prover.generate_parameters_from_lagrange(mats, lag)
    from_lagrange_wall = time.perf_counter() - t0
    products_ms = prover.lagrange_timings()["products_ms"]
    for f in KEY_FIELDS:
        assert (getattr(got, f) == getattr(want, f)).all(), f"{f}: the key from the Lagrange form differs from the key from the SRS"

    line = dict(tool="lagrange_bench", curve=curve, k=k, domain=n, qap=args.qap, chunk=int(os.environ.get("G16_LAGRANGE_CHUNK", 1 << 17)),
                cpus=len(os.sched_getaffinity(0)), device=torch.cuda.get_device_name(args.device), keys_equal=True,
                srs_from_trapdoor_s=round(t_srs, 3), prepare_srs_wall_s=round(prepare_wall, 3),
                **{"prepare_" + name: round(v, 3) for name, v in ev.items() if name != "products_ms"},
                prepare_transforms_ms=round(new_transforms_ms, 3), from_srs_transforms_ms=round(old["transforms_ms"], 3),
                transforms_old_over_new=round(old["transforms_ms"] / new_transforms_ms, 3), from_srs_h_ms=round(old["h_ms"], 3),
                from_srs_products_ms=round(old["products_ms"], 3), from_srs_wall_s=round(from_srs_wall, 3),
                from_lagrange_wall_s=round(from_lagrange_wall, 3), from_lagrange_products_ms=round(products_ms, 3),
                key_from_srs_over_key_from_lagrange=round(from_srs_wall / from_lagrange_wall, 2))
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    prover.close()


if __name__ == "__main__":
    main()
