#!/usr/bin/env python3
"""Headline benchmark: R1CS constraints/second of create_proof (BLS12-381) on N x MI355X.

A "step" is one Groth16 proof of the synthetic R1CS SYN(k) (Fibonacci product chain,
n_c = 2^k - 2 constraints, FFT domain exactly 2^k; default k = 22 = BASELINE.json configs[2], the full
prover: witness-map NTTs + h/l/a/b_g1 G1 MSMs + the b_g2 G2 MSM) over a VALID proving key generated on the
GPU from seeded toxic waste (g16_generate_parameters = Groth16::generate_parameters_with_qap; --key synthetic
falls back to distinct non-identity points), with the witness, the CSR matrices and the proving key already
resident in HBM when the timed region starts -- the scope of
Groth16::create_proof_with_reduction_and_matrices (/root/reference/src/prover.rs:26-51).

N > 1 (one process per GPU, launched by torch.distributed.run): the MSM base arrays are sharded over
the ranks (strong scaling: the SAME proof), the witness map is distributed too (g16_dwm_*: every n-point transform as a
local n/N-point transform, a twiddle, ONE all-to-all over RCCL and a local N-point transform; h stays in the block
distribution its h_query shard is gathered in), every rank computes its partial sums, ONE all-gather of the 1.2 KB
partial records over RCCL combines them and every rank finishes the proof.

Prints one JSON line on rank 0.  A plain run only sets up, warms up, times --steps proofs and reports the headline (value,
ms_per_step, the per-phase timers of the timed steps).  --full adds, after the timed steps, everything that needs work of its own:
  roofline      dominant kernel (the G1 bucket-accumulation pass) against the 8 TB/s HBM roofline (+ roofline_ntt)
  cpu_baseline  the CPU oracle (C++ restatement of ark-groth16's algorithm, NOT ark-groth16 itself) timed
                on the host cores on a bounded sample (smaller k), rank 0, N = 1 only
  value_incl_h2d, projected_scaling, pipelined (N = 1); collective_ms, configs4 (N > 1)
--dump-outputs DIR writes the proof of the last timed step (what a caller of the prover receives) as .npy files.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import groth16_amd as g  # noqa: E402
from groth16_amd.binding import (CURVE_ID, FQ_LIMBS, CsrViewC, DiagC, ParamsViewC, PartialC, PkInfoC, PkViewC, ProofC, QueryC, TimingsC,  # noqa: E402
                                 ToxicWasteC, ptr32, ptr64)
from groth16_amd.groth16 import _MODULUS_R, DistributedWitnessMap, bucket_h_indices, dist_h_indices  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def shard_range(n, idx, cnt):
    return n * idx // cnt, n * (idx + 1) // cnt


class DeviceProver:
    """SYN(k) circuit + this rank's part of the proving key, everything resident on one GPU.  key = "valid": the CRS of the circuit,
    generated on the GPU from seeded toxic waste; "synthetic": distinct non-identity points (any points give the same prover work).
    mode = "base": the rank holds a contiguous range of every MSM base array; "bucket": the WHOLE key as window tables and the
    buckets b mod world == rank of every MSM (g16_pk_load_bucket_shard)."""

    def __init__(self, curve, k, seed, rank, world, device, key="valid", dist_wm=False, mode="base"):
        """dist_wm: this rank runs its part of the distributed witness map and holds h_query in the order its h arrives in"""
        self.curve, self.k, self.rank, self.world, self.key = curve, k, rank, world, key
        self.mode = mode if world > 1 else "base"
        self.sim = False   # --sim-shards: the h all-gather of a bucket-space shard is simulated by local copies
        self.dwm, self.dwm_ms = None, 0.0
        self.lib = g.lib()
        c = self.lib.c
        L = FQ_LIMBS[curve]
        self.L = L
        self.device = device
        self.ctx = C.c_void_p()
        self.lib.check(c.g16_ctx_create(CURVE_ID[curve], device, C.byref(self.ctx)))
        nc = (1 << k) - 2
        self.nc, self.nin, self.nvars = nc, 2, nc + 3
        self.n = 1 << k
        # ---- circuit + witness (host generator in the product library), then to HBM
        z = np.zeros((self.nvars, 4), dtype=np.uint64)
        rp = np.zeros(nc + 1, dtype=np.uint64)
        cols = [np.zeros(nc, dtype=np.uint32) for _ in range(3)]
        val = np.zeros((nc, 4), dtype=np.uint64)
        self.lib.check(c.g16_synth_circuit(CURVE_ID[curve], k, seed, ptr64(z), ptr64(rp), ptr32(cols[0]), ptr32(cols[1]),
                                           ptr32(cols[2]), ptr64(val)))
        self.z_host, self.csr_host = z, (rp, cols, val)
        self._views = (CsrViewC * 3)(*[CsrViewC(ptr64(rp), ptr32(cols[i]), ptr64(val)) for i in range(3)])
        self.ck = C.c_void_p()
        self.lib.check(c.g16_circuit_load(self.ctx, self._views, self.nin, nc, self.nvars, C.byref(self.ck)))
        self.z_dev = torch.from_numpy(z.view(np.int64)).to(f"cuda:{device}")
        self.seed = seed
        self.seeds = dict(a=101, b1=102, b2=103, h=104, l=105, fixed1=106, fixed2=107)
        self._full = None
        self.fixed = None
        # ---- this rank's part of the proving key: bases generated straight into HBM
        self.pk, self.bufs, self.ranges, self.pk_load_s = self.load_key(rank, world, self.mode, dist_wm)
        if dist_wm:
            self.dwm = DistributedWitnessMap(self.lib, self.ctx, self.ck, rank, world, f"cuda:{device}")
        # fixed non-zero r, s (zero-knowledge randomness is an input: prover.rs:173-178)
        self.r = z[2].copy()
        self.s = z[3].copy()

    def _synth(self, g2, sd, first, cnt):
        words = (4 if g2 else 2) * self.L
        t = torch.empty((max(cnt, 1), words), dtype=torch.int64, device=f"cuda:{self.device}")
        self.lib.check(self.lib.c.g16_synth_bases(self.ctx, int(g2), sd, first, cnt, C.c_void_p(t.data_ptr())))
        return t

    def _generate_valid_key(self):
        """Groth16::generate_parameters_with_qap (generator.rs:47-208) straight into HBM; every rank derives the same key from the
        same seed and keeps its part"""
        c, L, dev = self.lib.c, self.L, f"cuda:{self.device}"
        hlen, w = self.n - 1, self.nvars - self.nin
        rs = np.random.RandomState(20240 + self.seed)
        mod = _MODULUS_R[self.curve]

        def rand_fr():
            v = int.from_bytes(rs.bytes(64), "little") % mod or 1
            v = (v << 256) % mod   # Montgomery form
            return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]

        tw = ToxicWasteC()
        for name in ("alpha", "beta", "gamma", "delta", "t"):
            getattr(tw, name)[:] = rand_fr()
        gen1 = self._synth(False, self.seeds["fixed1"], 0, 1).cpu().numpy().view(np.uint64).reshape(-1).copy()
        gen2 = self._synth(True, self.seeds["fixed2"], 0, 1).cpu().numpy().view(np.uint64).reshape(-1).copy()
        full = dict(a=torch.empty((self.nvars, 2 * L), dtype=torch.int64, device=dev),
                    b1=torch.empty((self.nvars, 2 * L), dtype=torch.int64, device=dev),
                    b2=torch.empty((self.nvars, 4 * L), dtype=torch.int64, device=dev),
                    h=torch.empty((hlen, 2 * L), dtype=torch.int64, device=dev), l=torch.empty((w, 2 * L), dtype=torch.int64, device=dev))
        fx = dict(alpha_g1=np.zeros(2 * L, dtype=np.uint64), beta_g1=np.zeros(2 * L, dtype=np.uint64), delta_g1=np.zeros(2 * L, dtype=np.uint64),
                  beta_g2=np.zeros(4 * L, dtype=np.uint64), delta_g2=np.zeros(4 * L, dtype=np.uint64))
        self.vk_rest = dict(gamma_g2=np.zeros(4 * L, dtype=np.uint64), gamma_abc_g1=np.zeros((self.nin, 2 * L), dtype=np.uint64))
        out = ParamsViewC(ptr64(fx["alpha_g1"]), ptr64(fx["beta_g1"]), ptr64(fx["delta_g1"]), ptr64(fx["beta_g2"]), ptr64(fx["delta_g2"]),
                          ptr64(self.vk_rest["gamma_g2"]), ptr64(self.vk_rest["gamma_abc_g1"]), C.c_void_p(full["a"].data_ptr()),
                          C.c_void_p(full["b1"].data_ptr()), C.c_void_p(full["b2"].data_ptr()), C.c_void_p(full["h"].data_ptr()),
                          C.c_void_p(full["l"].data_ptr()), 1)
        self.lib.check(c.g16_generate_parameters(self.ctx, self._views, self.nin, self.nc, self.nvars, C.byref(tw), ptr64(gen1), ptr64(gen2),
                                                 C.byref(out)))
        u64 = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1).copy()  # noqa: E731
        fx.update(a0=u64(full["a"][0]), b10=u64(full["b1"][0]), b20=u64(full["b2"][0]))
        self.fixed = fx
        self._full = full

    def load_key(self, rank, world, mode, dist_wm):
        """rank's part of the key under `mode` onto the GPU: (g16_pk handle, the standard-form bases it was built from, the index
        ranges, seconds of g16_pk_load).  The headline prover calls it once; the projected-scaling leg again per simulated cut."""
        c, L, dev = self.lib.c, self.L, f"cuda:{self.device}"
        bucket = mode == "bucket" and world > 1
        m, w, hlen = self.nvars - 1, self.nvars - self.nin, self.n - 1
        a_lo, a_hi = (0, m) if bucket else shard_range(m, rank, world)
        l_lo = min(w, max(0, a_lo - (self.nin - 1)))
        l_hi = min(w, max(0, a_hi - (self.nin - 1)))
        h_lo, h_hi = (0, hlen) if bucket else shard_range(hlen, rank, world)
        h_sel = None
        if dist_wm:
            # h_query in the order the distributed map leaves h in: this rank's block (base-range shard), or -- bucket-space shard:
            # every rank folds ALL of h -- the ranks' blocks back to back, as the all-gather delivers them (the last index, n - 1,
            # has no base)
            idx = bucket_h_indices(self.n, world) if bucket else dist_h_indices(self.n, rank, world)
            h_sel = torch.from_numpy(idx[idx < hlen]).to(dev)
            h_lo, h_hi = 0, int(h_sel.numel())
        ranges = dict(a=(a_lo, a_hi), l=(l_lo, l_hi), h=(h_lo, h_hi))
        if self.key == "valid":
            if self._full is None:
                self._generate_valid_key()
            full = self._full
            bufs = dict(a=full["a"][1 + a_lo: 1 + a_hi], b1=full["b1"][1 + a_lo: 1 + a_hi], b2=full["b2"][1 + a_lo: 1 + a_hi],
                        h=full["h"][h_lo: h_hi] if h_sel is None else full["h"].index_select(0, h_sel), l=full["l"][l_lo: l_hi])
        else:
            # index 0 of the a/b generators is query[0]; MSM index i is generator index 1 + i
            sy, sd = self._synth, self.seeds
            bufs = dict(
                a=sy(False, sd["a"], 1 + a_lo, a_hi - a_lo), b1=sy(False, sd["b1"], 1 + a_lo, a_hi - a_lo),
                b2=sy(True, sd["b2"], 1 + a_lo, a_hi - a_lo),
                h=sy(False, sd["h"], h_lo, h_hi - h_lo) if h_sel is None else sy(False, sd["h"], 0, hlen).index_select(0, h_sel),
                l=sy(False, sd["l"], l_lo, l_hi - l_lo))
            if self.fixed is None:
                q0a = sy(False, sd["a"], 0, 1).cpu().numpy().view(np.uint64).reshape(-1)
                q0b1 = sy(False, sd["b1"], 0, 1).cpu().numpy().view(np.uint64).reshape(-1)
                q0b2 = sy(True, sd["b2"], 0, 1).cpu().numpy().view(np.uint64).reshape(-1)
                f1 = sy(False, sd["fixed1"], 0, 3).cpu().numpy().view(np.uint64)  # alpha_g1, beta_g1, delta_g1
                f2 = sy(True, sd["fixed2"], 0, 2).cpu().numpy().view(np.uint64)   # beta_g2, delta_g2
                self.fixed = dict(alpha_g1=f1[0].copy(), beta_g1=f1[1].copy(), delta_g1=f1[2].copy(), beta_g2=f2[0].copy(),
                                  delta_g2=f2[1].copy(), a0=q0a.copy(), b10=q0b1.copy(), b20=q0b2.copy())

        def q(t, lo, hi):
            return QueryC(t.data_ptr() if hi > lo else None, hi - lo, lo)

        fx = self.fixed
        view = PkViewC(ptr64(fx["alpha_g1"]), ptr64(fx["beta_g1"]), ptr64(fx["delta_g1"]), ptr64(fx["beta_g2"]), ptr64(fx["delta_g2"]),
                       ptr64(fx["a0"]), ptr64(fx["b10"]), ptr64(fx["b20"]), q(bufs["a"], a_lo, a_hi), q(bufs["b1"], a_lo, a_hi),
                       q(bufs["b2"], a_lo, a_hi), q(bufs["h"], h_lo, h_hi), q(bufs["l"], l_lo, l_hi), 1)
        pk = C.c_void_p()
        torch.cuda.synchronize()
        t_load = time.perf_counter()
        if bucket:
            self.lib.check(c.g16_pk_load_bucket_shard(self.ctx, C.byref(view), rank, world, C.byref(pk)))
        else:
            self.lib.check(c.g16_pk_load(self.ctx, C.byref(view), C.byref(pk)))
        # the "cold" cost: window tables built from device-resident bases, once per key.  `bufs`: standard-form copies kept for the
        # CPU-baseline download (the library holds its own)
        return pk, bufs, ranges, time.perf_counter() - t_load

    def pk_info(self):
        out = PkInfoC()
        self.lib.check(self.lib.c.g16_pk_get_info(self.pk, C.byref(out)))
        return out.as_dict()

    def partial(self, host_z=None, dist=None):
        """host_z = None: the witness is already in HBM (the timed configuration); else a host pointer (int) to upload from.
        With the distributed witness map: its four stages + three exchanges over `dist` first, then the MSMs over this rank's h block."""
        part = PartialC()
        zp = C.c_void_p(self.z_dev.data_ptr()) if host_z is None else C.c_void_p(host_z)
        if not os.environ.get("G16_BENCH_NO_FIN_PREPARE"):   # the (r, s)-only host glue runs on a host thread under the GPU work
            self.lib.check(self.lib.c.g16_prove_finalize_prepare(self.ctx, self.pk, ptr64(self.r), ptr64(self.s)))
        if self.dwm is not None:
            t0 = time.perf_counter()
            if host_z is None and not os.environ.get("G16_BENCH_NO_PREPARE"):   # the witness sort goes into the queues ahead of the map's stages
                self.lib.check(self.lib.c.g16_prove_partial_prepare(self.ctx, self.pk, self.ck, zp, self.nvars))
            h = self.dwm.run(self.z_dev.data_ptr() if host_z is None else host_z, self.nvars, host_z is None, dist)
            h_len = self.dwm.M
            if self.mode == "bucket" and self.world > 1:
                # a bucket-space shard folds ALL of h: one all-gather of the ranks' blocks (RCCL over xGMI; n / world Fr per rank)
                h = self.dwm.all_gather_h(dist, simulate=self.sim)
                h_len = self.dwm.M * self.world
            self.dwm_ms = 1e3 * (time.perf_counter() - t0)
            self.lib.check(self.lib.c.g16_prove_partial_h(self.ctx, self.pk, self.ck, zp, self.nvars, 1 if host_z is None else 0,
                                                          C.c_void_p(h.data_ptr()), h_len, 0, C.byref(part)))
            return part
        self.lib.check(self.lib.c.g16_prove_partial(self.ctx, self.pk, self.ck, zp, self.nvars, 1 if host_z is None else 0, 0, C.byref(part)))
        return part

    def finalize(self, parts):
        arr = (PartialC * len(parts))(*parts)
        out = ProofC()
        self.lib.check(self.lib.c.g16_prove_finalize(self.ctx, self.pk, arr, len(parts), ptr64(self.r), ptr64(self.s), C.byref(out)))
        L = self.L
        return np.concatenate([np.array(out.a[: 2 * L], dtype=np.uint64), np.array(out.b[: 4 * L], dtype=np.uint64),
                               np.array(out.c[: 2 * L], dtype=np.uint64)])

    def timings(self):
        t = TimingsC()
        self.lib.check(self.lib.c.g16_get_timings(self.ctx, C.byref(t)))
        return t.as_dict()

    def close(self):
        """give the HBM back (window tables, circuit, arena) -- the configs[4] leg loads a 2^24 shard after the 2^22 one"""
        if self.dwm is not None:
            self.dwm.close()
            self.dwm = None
        if self.pk:
            self.lib.c.g16_pk_free(self.pk)
            self.pk = None
        if self.ck:
            self.lib.c.g16_circuit_free(self.ck)
            self.ck = None
        if self.ctx:
            self.lib.c.g16_ctx_destroy(self.ctx)
            self.ctx = None
        self.bufs = self._full = self.z_dev = None
        torch.cuda.empty_cache()


def prove_step(p, dist, device):
    part = p.partial(dist=dist)
    if dist is None:
        return p.finalize([part])
    t = torch.frombuffer(bytearray(bytes(part)), dtype=torch.uint8).to(device)
    outs = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(outs, t)  # RCCL over xGMI: ~1.2 KB per rank, one collective per proof
    parts = [PartialC.from_buffer_copy(o.cpu().numpy().tobytes()) for o in outs]
    return p.finalize(parts)


def dump_proof(dirname, proof, L):
    """the proof as np.save files a later build's can be compared with element for element: each u64 Montgomery limb as its two u32
    words (little-endian), float64 holds them exactly; a: 2 x 2L, b: 4 x 2L (x.c0, x.c1, y.c0, y.c1), c: 2 x 2L"""
    os.makedirs(dirname, exist_ok=True)
    words = proof.view(np.uint32).astype(np.float64).reshape(-1, 2 * L)
    for name, rows in (("a", words[:2]), ("b", words[2:6]), ("c", words[6:])):
        np.save(os.path.join(dirname, f"proof_{name}.npy"), rows)


def cpu_quota():
    """CPUs this container may actually burn (cgroup cpu.max), or None when unlimited -- `cores` in the cpu_baseline object is the
    number of OpenMP THREADS used; on a quota-limited box that is more than the CPUs they get"""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if quota == "max" else round(int(quota) / int(period), 2)
    except Exception:  # noqa: BLE001
        return None


def pipelined_throughput(p, device, proofs_per_ctx, want_proof):
    """THROUGHPUT mode (reported beside the headline, never instead of it): a second context on the same GPU sharing the key, the
    circuit and the witness already in HBM; two host threads prove back to back, the second one starting half a proof later, so the
    head (witness map, sort) and tail (reductions, host glue) of one proof run under the bucket passes of the other.  Every proof
    is compared with the headline proof."""
    import threading

    lib, c = p.lib, p.lib.c
    ctx2 = C.c_void_p()
    lib.check(c.g16_ctx_create(CURVE_ID[p.curve], device, C.byref(ctx2)))
    zp = C.c_void_p(p.z_dev.data_ptr())
    L = p.L
    bad, done = [], [0, 0]

    def one(ctx):
        out = ProofC()
        lib.check(c.g16_prove(ctx, p.pk, p.ck, zp, p.nvars, 1, ptr64(p.r), ptr64(p.s), C.byref(out)))
        return np.concatenate([np.array(out.a[: 2 * L], dtype=np.uint64), np.array(out.b[: 4 * L], dtype=np.uint64),
                               np.array(out.c[: 2 * L], dtype=np.uint64)])

    def worker(k, ctx, delay_s, n):
        try:
            if delay_s:
                time.sleep(delay_s)
            for _ in range(n):
                if not (one(ctx) == want_proof).all():
                    bad.append(k)
                done[k] += 1
        except Exception as e:  # noqa: BLE001
            bad.append(repr(e))

    try:
        one(ctx2)   # warm-up of the second context (arena, pinned buffer, function attributes)
        one(p.ctx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        one(p.ctx)
        solo = time.perf_counter() - t1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        th = [threading.Thread(target=worker, args=(0, p.ctx, 0.0, proofs_per_ctx)),
              threading.Thread(target=worker, args=(1, ctx2, solo / 2, proofs_per_ctx))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        c.g16_ctx_destroy(ctx2)
    n = done[0] + done[1]
    return dict(contexts=2, proofs=n, seconds=dt, ms_per_proof=1e3 * dt / max(n, 1), value=p.nc * n / dt, unit="constraints/s",
                every_proof_equals_headline_proof=not bad and n == 2 * proofs_per_ctx,
                note="two contexts on one GPU over one key, two host threads, g16_prove back to back, the second offset by half a proof; "
                     "latency per proof roughly doubles, the chip stays full through heads and tails")


def default_cpu_threads():
    """the GPU box's container is CPU-quota limited (cgroup cpu.max); oversubscribing the OpenMP oracle past ~2x the
    quota collapses its throughput (measured: tools/cpu_thread_sweep.py), so use 2x quota, else all CPUs"""
    ncpu = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            return max(1, min(ncpu, int(round(2 * int(quota) / int(period)))))
    except Exception:  # noqa: BLE001
        pass
    return ncpu


def cpu_baseline(curve, k_cpu, seed, threads, key="valid", reuse=None):
    """CPU oracle on a bounded sample: same circuit family / key shape at k_cpu; pk generated on the GPU and
    downloaded so that GPU and CPU prove the very same instance (also a parity check of this bench).  `reuse`: the
    benchmark's own DeviceProver when the sample IS the benchmark instance (--cpu-log2 == --log2)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import Csr, FlatCircuit, FlatPk, oracle

    orc = oracle()
    orc.set_threads(threads or default_cpu_threads())
    dp = reuse if reuse is not None else DeviceProver(curve, k_cpu, seed, 0, 1, torch.cuda.current_device(), key)
    gpu_proof = dp.finalize([dp.partial()])
    rp, cols, val = dp.csr_host
    ck = FlatCircuit(curve, dp.nin, dp.nc, dp.nvars, [Csr(rp, cols[i], val) for i in range(3)], dp.z_host)

    def host(t):
        return np.ascontiguousarray(t.cpu().numpy().view(np.uint64))

    fx = dp.fixed
    pk = FlatPk(curve, fx["alpha_g1"][None, :], fx["beta_g1"][None, :], fx["delta_g1"][None, :], fx["beta_g2"][None, :],
                fx["delta_g2"][None, :], np.concatenate([fx["a0"][None, :], host(dp.bufs["a"])]),
                np.concatenate([fx["b10"][None, :], host(dp.bufs["b1"])]), np.concatenate([fx["b20"][None, :], host(dp.bufs["b2"])]),
                host(dp.bufs["h"]), host(dp.bufs["l"]))
    t0 = time.time()
    proof, phases = orc.prove(pk, ck, dp.r, dp.s)
    dt = time.time() - t0
    match = bool((proof == gpu_proof).all())
    return dict(value=dp.nc / dt, unit="constraints/s", cores=orc.threads, threads=orc.threads, cpu_quota=cpu_quota(),
                host_cpus=os.cpu_count(), kind="port",
                sample=f"SYN(k={k_cpu}) {curve}, {dp.nc} constraints, one proof, {dt:.2f} s; C++ restatement of ark-groth16's "
                       f"CPU algorithm (oracle/g16_oracle.cpp), not ark-groth16 itself",
                seconds=dt, phases={k_: round(v, 3) for k_, v in phases.items()}, gpu_proof_matches_cpu=match)


def sim_share(p, n_ranks, mode, steps, warmup, use_dwm, ranks=(0,)):
    """DIAGNOSTIC: one rank's share of an n_ranks-way sharded proof, measured on THIS GPU -- the rank's stages of the distributed witness
    map with the exchanges (and a bucket-space shard's h all-gather) replaced by device copies of the same size, its five partial sums,
    then the finalize over n_ranks records.  RCCL / xGMI latencies are NOT in it.  mode "bucket" re-labels the resident whole-key tables
    (g16_pk_rebind_bucket_shard: they do not depend on the rank) when p holds them; otherwise the shard is loaded from the key
    material in HBM and freed again.  Returns the slowest of `ranks`."""
    lib, c = p.lib, p.lib.c
    saved = (p.pk, p.dwm, p.rank, p.world, p.mode, p.sim, p.bufs, p.ranges)
    whole = p.world == 1 or p.mode == "bucket"
    rebind = mode == "bucket" and whole and p.pk_info()["window_bits_z"] > 0
    worst = None
    try:
        for r in ranks:
            dwm = pk = None
            try:
                if rebind:
                    lib.check(c.g16_pk_rebind_bucket_shard(saved[0], r, n_ranks))
                    pk, load_s = saved[0], 0.0
                else:
                    pk, p.bufs, p.ranges, load_s = p.load_key(r, n_ranks, mode, use_dwm)
                if use_dwm:
                    dwm = DistributedWitnessMap(lib, p.ctx, p.ck, r, n_ranks, f"cuda:{p.device}")
                p.pk, p.dwm, p.rank, p.world, p.mode, p.sim = pk, dwm, r, n_ranks, mode, True
                for _ in range(warmup):
                    p.partial()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    part = p.partial()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / steps
                t1 = time.perf_counter()
                p.finalize([part] * n_ranks)   # (picks up the (r, s)-only half the last partial() started: the real flow)
                fin = time.perf_counter() - t1
                got = dict(rank=r, partial_ms=1e3 * dt, finalize_ms=1e3 * fin, phases=p.timings(), pk_load_s=round(load_s, 3),
                           enqueue_ms=p.dwm_ms if dwm is not None else None)
                if worst is None or got["partial_ms"] > worst["partial_ms"]:
                    worst = got
            finally:
                if dwm is not None:
                    dwm.close()
                if pk is not None and not rebind:
                    c.g16_pk_free(pk)
    finally:
        p.pk, p.dwm, p.rank, p.world, p.mode, p.sim, p.bufs, p.ranges = saved
        if rebind:
            lib.check(c.g16_pk_rebind_bucket_shard(p.pk, p.rank if p.mode == "bucket" else 0, p.world if p.mode == "bucket" else 1))
    return worst


def projected_scaling(p, single_ms, steps, dist_wm_ok):
    """PROJECTION, not a measurement of N GPUs (none has been available to this repository): per-rank share of the SAME proof at 2, 4, 8
    ranks under both ways of cutting the MSMs, each measured on this one GPU (sim_share), and single_ms / share.  What it leaves out:
    RCCL latency of the map's 7 all-to-all calls, of the h all-gather (bucket mode) and of the record all-gather."""
    out = dict(note="projection from ONE GPU: rank share = the rank's own stages with every exchange replaced by a device copy of the same "
                    "bytes; no RCCL / xGMI latency; projected_speedup = single-GPU ms_per_step / (partial_ms + finalize_ms)",
               single_gpu_ms=single_ms, points=[])
    for mode in ("bucket", "base"):
        for n_ranks in (2, 4, 8):
            try:
                ranks = tuple(range(n_ranks)) if mode == "bucket" else (0,)
                sh = sim_share(p, n_ranks, mode, max(2, min(steps, 4)), 2, dist_wm_ok(n_ranks, p.k), ranks)
                share = sh["partial_ms"] + sh["finalize_ms"]
                out["points"].append(dict(n_gpus=n_ranks, shard_mode=mode, rank_share_ms=round(share, 3), partial_ms=round(sh["partial_ms"], 3),
                                          finalize_ms=round(sh["finalize_ms"], 3), projected_speedup=round(single_ms / share, 3),
                                          projected_value=p.nc / (share * 1e-3), ranks_measured=len(ranks),
                                          bucket_pass_ms=round(sh["phases"]["bucket_pass_ms"], 3),
                                          window_bits=int(sh["phases"]["window_bits"]), windows=int(sh["phases"]["windows"])))
            except Exception as e:  # noqa: BLE001 -- a projection must never take the headline line down
                out["points"].append(dict(n_gpus=n_ranks, shard_mode=mode, error=repr(e)))
    return out


def pick_shard_mode(want, world, k, curve, device, dist):
    """how the MSMs are cut over the ranks.  auto: bucket-space shards (whole window tables on every GPU, buckets divided: the bucket
    reductions shrink with the rank count too) whenever the tables of the WHOLE key fit in this GPU's free HBM with room for the
    per-proof arena, else base-range shards (1 / world of the tables per GPU).  Every rank must decide alike: MIN over the ranks."""
    if world == 1:
        return "base", "single GPU"
    why = f"--shard-mode {want}"
    mode = want
    if want == "auto":
        g1 = 2 * FQ_LIMBS[curve] * 8
        key_bytes = (1 << k) * 6 * g1                     # a, b_g1, l, h (G1) + b_g2 (G2 = 2 G1)
        rows = 13 if k >= 20 else 32                      # window tables: W rows (c = 20: 13; small keys use small windows, more rows)
        need = int(rows * key_bytes * 1.08) + 3 * key_bytes + (8 << 30)
        free, _total = torch.cuda.mem_get_info(device)
        # ... and only while the whole key's tables stay below ~80 GiB: at 2^24 (126 GB) the passes of a bucket-space shard gather from
        # a table eight times the size of a base-range shard's and lose to address translation what the smaller reductions gain
        # (36.2 vs 36.4 ms per rank, same box) -- no reason to hold 8x the memory and load 8x as long for a tie
        mode = "bucket" if need < free and rows * key_bytes <= (80 << 30) else "base"
        why = f"auto: whole-key window tables need ~{need / 2**30:.0f} GiB, {free / 2**30:.0f} GiB free -> {mode}"
    if dist is not None and world > 1:
        flag = torch.tensor([1 if mode == "bucket" else 0], dtype=torch.int64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if mode == "bucket" and int(flag.item()) == 0:
            mode, why = "base", why + " (another rank cannot hold the whole key)"
    return mode, why


def run_configs4(args, dist, device, rank, world, local_rank, barrier, dist_wm_ok):
    """BASELINE.json configs[4]: synthetic R1CS with 2^24 constraints, BLS12-381, MSM bases sharded over the ranks (+ the
    distributed witness map), same timed bracket as the headline.  Every rank calls this; a rank whose setup fails reports it
    through an all-reduce BEFORE any data-path collective, so a failure yields {"error": ...} on every rank instead of a hang."""
    k4 = args.configs4_log2
    err, p4 = "", None
    try:
        # synthetic bases (generated on the GPU; any distinct points give the same prover work): the valid CRS of a 2^24 circuit costs
        # every rank ~15 s of HOST scalar work, eight ranks share one CPU quota, and this leg must not endanger the headline line
        mode4, why4 = pick_shard_mode(args.shard_mode, world, k4, args.curve, local_rank, None)   # no collective before the error protocol
        p4 = DeviceProver(args.curve, k4, 1, rank, world, local_rank, "synthetic", dist_wm=dist_wm_ok(world, k4), mode=mode4)
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        err = repr(e)
    # one all-reduce carries both "my setup worked" and "I hold a bucket-space shard": a rank that could not hold the whole key fails
    # its load (no silent fall-back in that mode), and ranks that disagree on the mode must not meet in a data-path collective
    ok = torch.tensor([0 if err else 1, 0 if err else (1 if p4.mode == "bucket" else 0), 0 if err else (0 if p4.mode == "bucket" else 1)],
                      dtype=torch.int64, device=device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok[0].item()) == 0 or (int(ok[1].item()) == 0 and int(ok[2].item()) == 0):
        if p4 is not None:
            p4.close()
        return {"error": err or ("setup failed on another rank" if int(ok[0].item()) == 0 else "ranks chose different shard modes")}
    steps, warmup = max(1, min(args.steps, 5)), max(1, min(args.warmup, 2))
    proof = None
    for _ in range(warmup):
        proof = prove_step(p4, dist, device)
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = prove_step(p4, dist, device)
    barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    pt = torch.from_numpy(proof.view(np.int64).copy()).to(device)
    gathered = [torch.empty_like(pt) for _ in range(world)]
    dist.all_gather(gathered, pt)
    same = all(bool((x == gathered[0]).all()) for x in gathered)
    import hashlib

    res = dict(workload=f"SYN(k={k4}) synthetic R1CS, {p4.nc} constraints, FFT domain 2^{k4}, {args.curve}, full create_proof, synthetic-bases proving key, "
                        + (f"MSM buckets sharded over {world} ranks (whole window tables per GPU)" if p4.mode == "bucket" else f"MSM bases sharded over {world} ranks")
                        + ((" + distributed witness map" + (" + h all-gather" if p4.mode == "bucket" else "")) if p4.dwm is not None else " (witness map replicated)"),
               shard_mode=p4.mode, shard_mode_reason=why4, pk=p4.pk_info(),
               log2_domain=k4, constraints=p4.nc, n_gpus=world, steps=steps, warmup=warmup, ms_per_step=1e3 * dt / steps,
               value=p4.nc * steps / dt, unit="constraints/s", pk_load_s=round(p4.pk_load_s, 3), ranks_agree_on_proof=same,
               proof_sha256=hashlib.sha256(proof.tobytes()).hexdigest(), phases_ms_rank0=p4.timings())
    p4.close()
    return res


def self_launch(n):
    """re-run this very command line under torch.distributed.run with n ranks on 127.0.0.1 (free port picked here); the
    children see WORLD_SIZE and take the normal path.  stdout / stderr are inherited: rank 0's JSON line is this process's."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on these hosts (RCCL needs it across processes)
    env.setdefault("OMP_NUM_THREADS", "1")              # what torchrun would set itself, without its warning on stderr
    return subprocess.call(cmd, env=env)


def roofline_objects(p, args, world, last_tm, bucket_g1, bucket_g2, phase_acc):
    """--full: the dominant kernel and the transforms against their bounds, from the timers of the timed steps (+ one run of
    g16_diag_valu's issue-rate kernel)"""
    # dominant kernel: the G1 bucket-accumulation pass (4 launches per proof).  Algorithmic bytes per launch =
    # N * (96 B affine base + 32 B scalar), N = points in this rank's shard.
    n_pts = p.ranges["a"][1] - p.ranges["a"][0]
    base_bytes = 2 * FQ_LIMBS[args.curve] * 8
    # (bucket-space shard: the rank folds 1 / world of the (point, window) entries of ALL points -- SURVEY 8(d): the sharded terms
    # divide by the GPU count)
    bucket_div = world if p.mode == "bucket" else 1
    # The G1 MSMs that are ready together share ONE launch of the kernel (l, a, b_g1; h too in a sharded proof): a "launch" below is
    # an actual launch (what rocprofv3 --stats averages over), its algorithmic bytes those of the MSMs it walks.
    g1_points = (p.ranges["h"][1] - p.ranges["h"][0]) + (p.ranges["l"][1] - p.ranges["l"][0]) + 2 * n_pts   # h, l, a, b_g1 (r != 0)
    g1_launches = max(1, int(round(last_tm.get("g1_pass_launches", 0))) or len([x for x in last_tm["bucket_ms"][:4] if x > 0]))
    g1_ms_per_step = float(np.sum(bucket_g1)) / args.steps if bucket_g1 else float("nan")
    alg_bytes = g1_points * (base_bytes + 32) // bucket_div // g1_launches
    avg_ms = g1_ms_per_step / g1_launches
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    # HBM bytes per launch from the PMC counters (separate rocprofv3 --pmc passes, committed under profiles/);
    # only valid for the workload they were collected on
    traffic, ntt_traffic, traffic_cal, traffic_src = None, None, None, None
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from tree_hash import kernel_source_sha16

        pt = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        wl = pt["workload"]
        here, there = kernel_source_sha16(ROOT), pt.get("kernel_source_sha16")
        if here != there:
            # counters of another tree say nothing about this one's kernels: not reported (re-collect: tools/gpu_session.sh <tag> pmc)
            traffic_src = (f"profiles/pmc_traffic.json was collected on kernel sources {there} (commit {pt.get('git_commit', '?')}), this run's "
                           f"are {here}: traffic withheld")
        elif wl["curve"] == args.curve and wl["log2_domain"] == args.log2 and wl["n_gpus"] == world:
            traffic_src = (f"profiles/pmc_traffic.json: rocprofv3 --pmc passes of this workload on THIS tree (kernel sources {here}, commit "
                           f"{pt.get('git_commit', '?')}); collected in their own run, not measured in this one")
            traffic = pt["hbm_bytes_per_launch"]
            ntt_traffic = pt.get("ntt_hbm_bytes_per_step")
            cal = pt.get("calibration")
            if cal:
                traffic_cal = (f"FETCH_SIZE x {cal['fetch']['factor']:.3f} ({cal['fetch']['pattern']}), WRITE_SIZE x {cal['write']['factor']:.3f} "
                               f"({cal['write']['pattern']}): factors of known-bytes kernels with the same access pattern run under the same "
                               "--pmc passes (tools/calib.hip, DESIGN.md 4.5)")
    except Exception:  # noqa: BLE001
        pass
    # the bound that actually applies: v_mad_u64_u32 issue.  Both sides of the fraction come from the library
    # (g16_diag_valu): the multiply-adds of one mixed addition counted from the kernels' own constexpr tables, and the
    # instruction's issue rate MEASURED on this GPU in this run (all CUs, 8 waves per SIMD, independent chains).
    n_windows = int(last_tm.get("windows", 0))
    valu = None
    if n_windows:
        dg = DiagC()
        p.lib.check(p.lib.c.g16_diag_valu(p.ctx, C.byref(dg)))
        mads = float(g1_points) * n_windows * dg.mads_per_add_g1 / bucket_div / g1_launches
        valu = dict(kind="v_mad_u64_u32 issue (integer VALU)", mads_per_launch=mads, achieved_Tmad_s=mads / (avg_ms * 1e-3) / 1e12,
                    measured_peak_Tmad_s=dg.mad_per_s / 1e12, frac=mads / (avg_ms * 1e-3) / dg.mad_per_s,
                    peak_source="g16_diag_valu: mad_rate_kernel timed in this run", mads_per_mixed_add=dg.mads_per_add_g1,
                    mads_per_field_product=dg.mads_per_product, limbs30=dg.limbs, window_bits=int(last_tm.get("window_bits", 0)),
                    windows=n_windows, points_folded_per_launch=g1_points * n_windows // bucket_div // g1_launches,
                    g2=dict(mads_per_mixed_add=dg.mads_per_add_g2, achieved_Tmad_s=float(n_pts) * n_windows * dg.mads_per_add_g2 / bucket_div /
                            (float(np.mean(bucket_g2)) * 1e-3) / 1e12 if bucket_g2 and np.mean(bucket_g2) > 0 else None))
    # second object for the transforms (2 * 32 * n algorithmic bytes per NTT, seven per proof), from the
    # HIP-event timers around them inside the witness map
    ntt_ms = phase_acc.get("ntt_ms", 0.0) / args.steps
    roofline_ntt = None
    if ntt_ms > 0:
        ntt_bytes = 7 * 2 * 32 * p.n
        roofline_ntt = dict(bound="hbm", achieved=ntt_bytes / (ntt_ms * 1e-3) / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                            frac=ntt_bytes / (ntt_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, kernel="ntt30_* (7 radix-2 transforms of size n per proof)",
                            ms_per_step=ntt_ms, algorithmic_bytes_per_step=ntt_bytes, traffic=ntt_traffic,
                            note="instruction-bound in practice (DESIGN.md 4.2); ms_per_step includes the pointwise quotient "
                                 "(a b - c) / Z, fused into the first sweep of the seventh transform since round 4 (it used to be a "
                                 "0.18 ms kernel outside this timer); replicated on every rank when sharded")
    roofline = dict(bound="hbm", achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s", frac=achieved / HBM_PEAK_GBS, traffic=traffic,
                    traffic_source=traffic_src,
                    traffic_calibration=traffic_cal,
                    binding_resource="integer VALU (v_mad_u64_u32 issue), not HBM: see valu_bound",
                    valu_bound=valu,
                    kernel="bucket_accumulate30_kernel (G1 Pippenger bucket pass)", launches_per_step=g1_launches,
                    avg_launch_ms=avg_ms, algorithmic_bytes_per_launch=alg_bytes,
                    msms_per_step=len(bucket_g1) // args.steps, per_msm_ms=g1_ms_per_step / max(1, len(bucket_g1) // args.steps),
                    launch_note="the G1 MSMs that are ready together go as ONE launch (one tail instead of one per MSM): avg_launch_ms and "
                                "algorithmic_bytes_per_launch are per ACTUAL launch (mean over launches of different size), per_msm_ms per MSM",
                    note="integer-VALU bound in practice (10 Fq products per 128 B); see DESIGN.md",
                    g2_bucket_avg_ms=float(np.mean(bucket_g2)))
    return roofline, roofline_ntt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, default=int(os.environ.get("G16_BENCH_LOG2", "22")))
    ap.add_argument("--curve", default="bls12_381")
    ap.add_argument("--cpu-log2", type=int, default=int(os.environ.get("G16_BENCH_CPU_LOG2", "0")),
                    help="size of the CPU-baseline sample; default (0) = --log2: the headline instance itself, ONE proof "
                         "(~25 s of CPU work at 2^22 on 16 cores), which also checks the GPU proof against the CPU prover's bit for bit")
    ap.add_argument("--cpu-threads", type=int, default=int(os.environ.get("G16_BENCH_CPU_THREADS", "0")))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipelined", action="store_true", help="skip the two-context throughput leg (reported as `pipelined`)")
    ap.add_argument("--key", choices=["valid", "synthetic", "auto"], default=os.environ.get("G16_BENCH_KEY", "auto"),
                    help="valid: CRS of the circuit generated on the GPU (g16_generate_parameters); synthetic: arbitrary distinct points "
                         "(the same prover work); auto (default): valid on one GPU, synthetic with N > 1 ranks -- a valid CRS costs every "
                         "rank ~10 s of HOST scalar work (Lagrange coefficients, the per-variable exponents), N ranks share one CPU quota, "
                         "and that untimed setup must not be what a driver's clock around an 8-rank run sees")
    ap.add_argument("--configs4", choices=["auto", "on", "off"], default=os.environ.get("G16_BENCH_CONFIGS4", "auto"),
                    help="with --full: after the headline line's timed region, also time BASELINE.json configs[4] (2^24 constraints, BLS12-381, "
                         "MSM bases sharded over the ranks) and report it as the `configs4` field of the same JSON line; auto = when --gpus "
                         "is 8 and --log2 is the headline 22")
    ap.add_argument("--configs4-log2", type=int, default=24, help=argparse.SUPPRESS)   # tests shrink it
    ap.add_argument("--shard-mode", choices=["auto", "base", "bucket"], default=os.environ.get("G16_BENCH_SHARD_MODE", "auto"),
                    help="N > 1: how the five MSMs are cut over the ranks -- base: contiguous ranges of the bases (1/N of the window tables per GPU); "
                         "bucket: the whole tables on every GPU, the BUCKETS divided (b mod N == rank), so the bucket reductions shrink with N "
                         "too; auto (default): bucket when the whole key's tables fit in free HBM, else base")
    ap.add_argument("--no-projection", action="store_true", help="N = 1: skip the projected_scaling leg (per-rank shares at 2 / 4 / 8 ranks "
                                                                  "measured on this GPU)")
    ap.add_argument("--sim-shards", type=int, default=0,
                    help="DIAGNOSTIC, not a benchmark: time one rank's share of an N-way sharded proof on a single GPU "
                         "(shard 0 of N, no exchange); the JSON line is tagged and must not be read as throughput")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything beside the headline: roofline objects, CPU baseline, "
                         "PCIe-inclusive rates, projected scaling, pipelined throughput (N = 1); collective timings, configs[4] (N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the proof of the last timed step to DIR/proof_{a,b,c}.npy (rank 0): the u32 words of its affine "
                         "Montgomery limbs as float64 (exact), shape (coordinates, words)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.configs4 == "on" and not args.full:
        ap.error("--configs4 on needs --full")
    if args.dump_outputs and args.sim_shards:
        ap.error("--dump-outputs writes the headline proof; --sim-shards computes none")
    if args.cpu_log2 <= 0:
        args.cpu_log2 = args.log2
    key_was_auto = args.key == "auto"
    if key_was_auto:
        args.key = "valid" if (args.gpus == 1 and not args.sim_shards) or os.environ.get("G16_BENCH_PRINT_PROOF") else "synthetic"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N` (no launcher): start the N ranks ourselves, one process per GPU, exactly as the
        # contract's `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...` would, and hand its exit code back
        sys.exit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}; run `python bench.py --gpus N` "
                 f"(self-launching) or torch.distributed.run with --nproc-per-node equal to --gpus")
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (there is no CPU fallback)"
    # test-only knobs (tests/test_gpu_parity.py::test_bench_two_ranks_one_gpu): run the N > 1 code path on a 1-GPU box by
    # putting every rank on device 0 and exchanging over gloo (RCCL refuses two ranks on one device)
    backend = os.environ.get("G16_BENCH_BACKEND", "nccl")
    if os.environ.get("G16_BENCH_FORCE_DEVICE0"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device(f"cuda:{local_rank}")
    dist = None
    # G16_BENCH_FORCE_DIST (test-only): take the collective path with a single rank too, so that the RCCL calls the N > 1 runs
    # make (process group on a device, all-gather / all-reduce / barrier on device tensors) can be exercised on a 1-GPU box
    if world > 1 or os.environ.get("G16_BENCH_FORCE_DIST"):
        import torch.distributed as dist_mod

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        import datetime

        # explicit collective timeout: a rank that dies in its (untimed, minutes at 2^24) setup must surface as an error on the others,
        # not as a silent wait for the default half hour
        tmo = datetime.timedelta(minutes=int(os.environ.get("G16_BENCH_COLLECTIVE_TIMEOUT_MIN", "20")))
        if backend == "nccl":
            dist_mod.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=device, timeout=tmo)
        else:
            dist_mod.init_process_group(backend=backend, rank=rank, world_size=world, timeout=tmo)
            device = torch.device("cpu")  # tensors handed to the collective live on the host for gloo
        dist = dist_mod
        if backend == "nccl":
            # the exchange of the distributed witness map is all_to_all_single on int64 [M, 4] device tensors: make sure this RCCL
            # build carries it (also with one rank, so that the 1-GPU test tier exercises the call the N > 1 runs depend on)
            probe = torch.arange(4 * 4 * world, dtype=torch.int64, device=device).reshape(4 * world, 4)
            got = torch.empty_like(probe)
            dist.all_to_all_single(got, probe)
            torch.cuda.synchronize()
            assert world > 1 or bool((got == probe).all()), "RCCL all_to_all_single returned wrong data"

    # proof that N ranks on N devices took part: every rank contributes (rank, device index, device uuid word, pid) through an
    # all-gather over the process group itself; rank 0 prints them
    ranks_seen = None
    if dist is not None:
        props = torch.cuda.get_device_properties(local_rank)
        uu = getattr(props, "uuid", None)
        uu_word = int.from_bytes(uu.bytes[:7], "little") if uu is not None else -1
        mine = torch.tensor([rank, local_rank, uu_word, os.getpid()], dtype=torch.int64, device=device)
        seen = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(seen, mine)
        ranks_seen = [dict(rank=int(x[0]), device=int(x[1]), device_uuid_word=f"{int(x[2]):014x}", pid=int(x[3])) for x in seen]
        # an N-rank number must come from N GPUs: a mis-pinned launch (LOCAL_RANK ignored, one visible device) fails HERE, on every
        # rank alike (all of them hold the same list), instead of printing an 8-rank line measured on fewer devices.  The test tier's
        # all-ranks-on-device-0 runs say so explicitly (G16_BENCH_FORCE_DEVICE0).
        n_distinct = len({(r_["device"], r_["device_uuid_word"]) for r_ in ranks_seen})
        if n_distinct < world and not os.environ.get("G16_BENCH_FORCE_DEVICE0"):
            if rank == 0:
                print(json.dumps({"error": f"{world} ranks on {n_distinct} distinct device(s): refusing to time a multi-GPU run", "ranks": ranks_seen}))
            dist.destroy_process_group()
            sys.exit(3)

    gpu = torch.device(f"cuda:{local_rank}")

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def dist_wm_ok(n_ranks, log2=None):
        """the distributed witness map needs a power-of-two rank count <= 16 with ranks^2 | domain size; G16_BENCH_DIST_WM=0
        keeps the replicated map (A/B)"""
        lw = n_ranks.bit_length() - 1
        if n_ranks == 1 and os.environ.get("G16_BENCH_FORCE_DWM"):   # test-only: the distributed-map path with a single rank
            return True
        return (n_ranks > 1 and (1 << lw) == n_ranks and n_ranks <= 16 and 2 * lw <= (log2 or args.log2) and
                os.environ.get("G16_BENCH_DIST_WM", "1") != "0")

    if args.sim_shards:
        assert world == 1
        mode, _why = pick_shard_mode(args.shard_mode, args.sim_shards, args.log2, args.curve, local_rank, None)   # auto: as N real ranks would
        use_dwm = dist_wm_ok(args.sim_shards)
        p = DeviceProver(args.curve, args.log2, 1, 0, args.sim_shards, local_rank, args.key, dist_wm=use_dwm, mode=mode)
        p.sim = True
        for _ in range(args.warmup):
            p.partial()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            part = p.partial()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        t1 = time.perf_counter()
        p.finalize([part] * args.sim_shards)   # (picks up the (r, s)-only half the last partial() started: the real flow)
        fin = time.perf_counter() - t1
        print(json.dumps({"diagnostic": "per-rank share of a sharded proof (NOT a throughput number)", "sim_shards": args.sim_shards,
                          "shard_mode": p.mode, "log2": args.log2, "partial_ms": 1e3 * dt, "finalize_ms": 1e3 * fin, "phases": p.timings(),
                          "pk": p.pk_info(), "pk_load_s": round(p.pk_load_s, 3),
                          "witness_map": ("distributed: rank 0's four stages, the three exchanges" +
                                          (" and the h all-gather" if p.mode == "bucket" else "") + " replaced by local copies, enqueued "
                                          f"without host synchronisation ({p.dwm_ms:.2f} ms of host time)") if p.dwm is not None else "replicated"}),
              flush=True)
        return
    t_setup = time.perf_counter()
    shard_mode, shard_why = pick_shard_mode(args.shard_mode, world, args.log2, args.curve, local_rank, dist)
    p = DeviceProver(args.curve, args.log2, 1, rank, world, local_rank, args.key, dist_wm=dist_wm_ok(world), mode=shard_mode)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t_setup
    proof = None
    for _ in range(args.warmup):
        proof = prove_step(p, dist, device)
    barrier()
    t0 = time.perf_counter()
    bucket_g1, bucket_g2, phase_acc, last_tm = [], [], {}, {}
    for _ in range(args.steps):
        proof = prove_step(p, dist, device)
        tm = last_tm = p.timings()  # event timers already resolved; no extra device work
        bucket_g1 += [x for x in tm["bucket_ms"][:4] if x > 0]
        bucket_g2.append(tm["bucket_ms"][4])
        for k_, v in tm.items():
            if k_ not in ("bucket_ms", "window_bits", "windows"):
                phase_acc[k_] = phase_acc.get(k_, 0.0) + v
        if p.dwm is not None:
            # host time to ENQUEUE the map's stages and exchanges (they run asynchronously on the library's witness-map stream)
            phase_acc["dist_witness_map_enqueue_ms"] = phase_acc.get("dist_witness_map_enqueue_ms", 0.0) + p.dwm_ms
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        # every rank must have produced the same proof
        pt = torch.from_numpy(proof.view(np.int64).copy()).to(device)
        gathered = [torch.empty_like(pt) for _ in range(world)]
        dist.all_gather(gathered, pt)
        assert all(bool((x == gathered[0]).all()) for x in gathered), "ranks disagree on the proof"
    if args.dump_outputs and rank == 0:
        dump_proof(args.dump_outputs, proof, p.L)

    # the collectives of one sharded proof, each timed ALONE after the timed steps (same tensors, same process group, HIP events on the
    # current stream, max over ranks): the terms a measured N > 1 line can be compared with the one-GPU projection by -- the projection
    # holds everything but these
    collective_ms = None
    if dist is not None and world > 1 and args.full:
        collective_ms = {}

        def time_coll(fn, reps=5):
            # host clock around `reps` calls with the device drained on both sides (works for RCCL and for the test tier's gloo, whose
            # tensors live on the host); the per-call launch overhead (~20 us) is inside
            fn()
            torch.cuda.synchronize()
            dist.barrier()
            t_a = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            t = torch.tensor([1e3 * (time.perf_counter() - t_a) / reps], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return round(float(t.item()), 4)

        rec = torch.zeros(C.sizeof(PartialC), dtype=torch.uint8, device=device)
        rec_out = [torch.empty_like(rec) for _ in range(world)]
        collective_ms["record_all_gather"] = time_coll(lambda: dist.all_gather(rec_out, rec))
        if p.dwm is not None:
            M = int(p.dwm.M)
            a2a_src = torch.zeros((M, 4), dtype=torch.int64, device=device)
            a2a_dst = torch.empty_like(a2a_src)
            one = time_coll(lambda: dist.all_to_all_single(a2a_dst, a2a_src))
            collective_ms["all_to_all_one_array"] = one
            collective_ms["all_to_all_per_proof_x7"] = round(7 * one, 4)
            if p.mode == "bucket":
                hparts = [torch.empty_like(a2a_src) for _ in range(world)]
                collective_ms["h_all_gather"] = time_coll(lambda: dist.all_gather(hparts, a2a_src))
                del hparts
            del a2a_src, a2a_dst
        collective_ms["note"] = ("each collective timed alone (5 calls back to back, host clock with the device drained, max over ranks); inside a proof they are "
                                 "enqueued on the witness-map stream beside the witness sort")

    # PCIe-inclusive rates (SURVEY.md 8(d) defines the metric with the witness on the host at entry; `value` above is the
    # HBM-resident rate the bench contract asks for): the same proof with full_assignment uploaded inside the call, from
    # pageable and from pinned host memory.  Outside the timed region; single-GPU only.
    h2d = None
    if dist is None and args.full:
        h2d = {}
        z_pinned = torch.from_numpy(p.z_host.view(np.int64)).pin_memory()
        for name, hp in (("pageable", p.z_host.ctypes.data), ("pinned", z_pinned.data_ptr())):
            p.finalize([p.partial(hp)])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            reps = max(2, min(args.steps, 5))
            for _ in range(reps):
                pr2 = p.finalize([p.partial(hp)])
            torch.cuda.synchronize()
            t_h = (time.perf_counter() - t1) / reps
            assert (pr2 == proof).all(), "host-witness proof differs from the device-witness proof"
            h2d[name] = dict(ms_per_step=1e3 * t_h, value=p.nc / t_h)

    # BASELINE.json configs[4] beside the headline (the driver passes no --log2): the SAME code path at 2^24 constraints, timed
    # with the same barrier / max-over-ranks bracket, reported as a field -- the headline `value` stays the 2^22 strong-scaling one
    want_c4 = args.full and dist is not None and (args.configs4 == "on" or (args.configs4 == "auto" and world == 8 and args.log2 == 22 and
                                                                              args.curve == "bls12_381"))
    out = None
    if rank == 0:
        ms_per_step = 1e3 * dt / args.steps
        value = p.nc * args.steps / dt
        out = {
            "metric": "R1CS constraints/sec (create_proof, BLS12-381)", "value": value, "unit": "constraints/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "u32-limb Montgomery integers (Fr 255-bit, Fq 381-bit)", "data": "synthetic",
            "config": {"workload": f"SYN(k={args.log2}) synthetic R1CS, {p.nc} constraints, FFT domain 2^{args.log2}, {args.curve}, "
                                   f"full create_proof (7 NTTs + 4 G1 MSMs + 1 G2 MSM), "
                                   + ("valid proving key generated on the GPU from seeded toxic waste" if args.key == "valid"
                                      else "synthetic-bases proving key"),
                       "curve": args.curve, "log2_domain": args.log2, "constraints": p.nc, "key": args.key,
                       "key_choice": ("auto: valid CRS on one GPU, synthetic bases with N > 1 ranks (bounds the untimed per-rank setup; any "
                                      "distinct points give the same prover work)") if key_was_auto else "--key",
                       "untimed_setup_s": round(t_setup, 2), "pk_load_s": round(p.pk_load_s, 3),
                       "witness": "resident in HBM at entry (--full: value_incl_h2d holds the PCIe-inclusive rates)",
                       "parallelism": ((f"msm-bucket-shard x{world} (whole window tables per GPU, buckets b mod {world} == rank)" if p.mode == "bucket"
                                        else f"msm-base-shard x{world}") +
                                       ((" + distributed witness map (3 all-to-all)" + (" + h all-gather" if p.mode == "bucket" else ""))
                                        if p.dwm is not None else " (witness map replicated)")) if world > 1 else "single-gpu",
                       "shard_mode": p.mode if world > 1 else None, "shard_mode_reason": shard_why if world > 1 else None,
                       # how the key is held: window tables, or plain bases and WHY (a slower prover: c <= 16, more windows)
                       "pk": p.pk_info()},
            "phases_ms_per_step": {k_: round(v / args.steps, 3) for k_, v in phase_acc.items()},
        }
        if args.full:
            out["roofline"], out["roofline_ntt"] = roofline_objects(p, args, world, last_tm, bucket_g1, bucket_g2, phase_acc)
            out["value_incl_h2d"] = h2d
            # SURVEY.md 8(d) defines the metric with the witness on the HOST at entry; the bench contract defines `value` with the
            # inputs resident in HBM.  Both are reported: `value` above (resident), this one with the 32 B x num_variables upload
            # from pinned host memory inside every timed call.
            out["value_survey_8d"] = (h2d or {}).get("pinned", {}).get("value")
        if dist is not None:
            out["rccl_world"] = dist.get_world_size()
            out["collective_backend"] = "rccl (torch.distributed nccl)" if backend == "nccl" else backend
            out["ranks"] = ranks_seen
            out["distinct_devices"] = len({(r_["device"], r_["device_uuid_word"]) for r_ in ranks_seen})
            if collective_ms is not None:
                out["collective_ms"] = collective_ms
        if args.full and world == 1 and not args.no_projection:
            try:
                out["projected_scaling"] = projected_scaling(p, ms_per_step, args.steps, dist_wm_ok)
                chk = p.finalize([p.partial()])   # the key is whole again (rebind undone): same proof as before
                out["projected_scaling"]["headline_proof_unchanged_after"] = bool((chk == proof).all())
            except Exception as e:  # noqa: BLE001
                out["projected_scaling"] = {"error": repr(e)}
        if args.full and world == 1 and not args.no_pipelined:
            try:
                out["pipelined"] = pipelined_throughput(p, local_rank, max(args.steps, 10), proof)
                out["value_pipelined"] = out["pipelined"]["value"]
            except Exception as e:  # noqa: BLE001 -- never take the headline line down
                out["pipelined"] = {"error": repr(e)}
        if os.environ.get("G16_BENCH_PRINT_PROOF"):
            import hashlib

            out["proof_sha256"] = hashlib.sha256(proof.tobytes()).hexdigest()
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args.curve, args.cpu_log2, 1, args.cpu_threads, args.key,
                                                   reuse=p if args.cpu_log2 == args.log2 else None)
            except Exception as e:  # noqa: BLE001 -- the baseline leg must never take the bench line down
                out["cpu_baseline"] = {"error": repr(e)}
    if want_c4:
        p.close()
        c4 = run_configs4(args, dist, device, rank, world, local_rank, barrier, dist_wm_ok)
        if rank == 0:
            out["configs4"] = c4
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
