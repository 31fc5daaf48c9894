#!/usr/bin/env python3
"""Time the two ways a serialized proving key reaches the GPU, in one process on one device:

  (a) host   serialize.proving_key_from_bytes (g16_deserialize_points on the host's threads) followed by g16_pk_load
  (b) device g16_pk_load_bytes: bytes uploaded, decoded and validated on the GPU, window tables built from the device arrays

The key is synthetic: SYN(k)'s shape (2^k + 1 / 2^k + 1 / 2^k + 1 / 2^k - 1 / 2^k - 1 points in a, b_g1, b_g2, h, l), bases generated
on the device (g16_synth_bases) and written out with g16_serialize_points.  Each path is warmed up and then timed `--reps` times;
the best is reported, with the stages of (b) from device events (g16_pk_load_bytes_timings).  One JSON line is appended to --out.

    python tools/key_load_bench.py --curve bls12_381 --k 18 --compressed 1 --validate 2 --out profiles/key_load_mi355x.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--curve", default="bls12_381", choices=["bls12_381", "bn254"])
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--compressed", type=int, default=1, choices=[0, 1])
    ap.add_argument("--validate", type=int, default=2, choices=[0, 1, 2])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("key_load_bench.py needs a GPU: a load is timed on the device or not at all")
    import groth16_amd as g
    import groth16_amd.serialize as ser
    from groth16_amd.groth16 import _DevicePk

    curve, k, compressed, validate = args.curve, args.k, bool(args.compressed), args.validate
    L = g.FQ_LIMBS[curve]
    nv, nh, nl = (1 << k) + 1, (1 << k) - 1, (1 << k) - 1
    prover = g.Groth16(curve, device=args.device)
    lb, ctx = g.lib(), prover._ctx

    def synth(g2, seed, n):
        t = torch.empty((n, (4 if g2 else 2) * L), dtype=torch.int64, device=f"cuda:{args.device}")
        lb.check(lb.c.g16_synth_bases(ctx.handle, int(g2), seed, 0, n, C.c_void_p(t.data_ptr())))
        torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint64)

    g1 = synth(False, 106, 5)
    g2 = synth(True, 107, 3)
    key = g.ProvingKey(curve, g1[0:1], g1[1:2], g1[2:3], g2[0:1], g2[1:2], synth(False, 101, nv), synth(False, 102, nv), synth(True, 103, nv),
                       synth(False, 104, nh), synth(False, 105, nl), g2[2:3], g1[3:5])
    t = time.perf_counter()
    data = ser.proving_key_to_bytes(curve, key, compressed)
    serialize_s = time.perf_counter() - t
    points = 3 * nv + nh + nl
    del key

    def host_path():
        t0 = time.perf_counter()
        back, used = ser.proving_key_from_bytes(curve, data, compressed, validate)
        t1 = time.perf_counter()
        dpk = _DevicePk(ctx, back, 2)   # g16_pk_load: returns once the tables are built
        t2 = time.perf_counter()
        info = dpk.info()
        dpk.close()
        assert used == len(data)
        return dict(decode_s=t1 - t0, pk_load_s=t2 - t1, total_s=t2 - t0), info

    def device_path():
        t0 = time.perf_counter()
        dkey = prover.load_proving_key_bytes(data, compressed, validate)   # returns once the tables are built
        t1 = time.perf_counter()
        ms = (C.c_double * 5)()
        lb.check(lb.c.g16_pk_load_bytes_timings(ms, 5))
        info = prover.pk_info(dkey, 2)
        assert dkey.consumed == len(data)
        prover.evict_pk(dkey)
        return dict(total_s=t1 - t0, walk_head_ms=ms[0], upload_ms=ms[1], decode_ms=ms[2], membership_fold_ms=ms[3], pk_load_ms=ms[4]), info

    runs = {"host": [], "device": []}
    infos = {}
    for rep in range(args.warmup + args.reps):   # alternating, so that neither path owns a quiet stretch of the machine
        for name, fn in (("host", host_path), ("device", device_path)):
            res, infos[name] = fn()
            if rep >= args.warmup:
                runs[name].append(res)
    assert infos["host"] == infos["device"], infos
    best = {name: min(rs, key=lambda r: r["total_s"]) for name, rs in runs.items()}
    line = dict(tool="key_load_bench", curve=curve, k=k, compressed=int(compressed), validate=validate, points=points, key_bytes=len(data),
                reps=args.reps, warmup=args.warmup, cpus=len(os.sched_getaffinity(0)), device=torch.cuda.get_device_name(args.device),
                serialize_s=round(serialize_s, 3), host=best["host"], device_path=best["device"],
                host_all_total_s=[round(r["total_s"], 4) for r in runs["host"]], device_all_total_s=[round(r["total_s"], 4) for r in runs["device"]],
                decode_speedup=round(best["host"]["decode_s"] / max(best["device"]["total_s"] - best["device"]["pk_load_ms"] / 1e3, 1e-9), 2),
                total_speedup=round(best["host"]["total_s"] / best["device"]["total_s"], 2), pk_info=infos["device"])
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
    prover.close()


if __name__ == "__main__":
    main()
