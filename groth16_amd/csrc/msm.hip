// Variable-base multi-scalar multiplication (Pippenger bucket method) for gfx950.
//
// Replaces ark-ec's VariableBaseMSM::msm_bigint at its five call sites in the prover
// (/root/reference/src/prover.rs:66, 74 and 262 via calculate_coeff :92,105,113).
// The reference runs one serial bucket scan per window, windows in parallel (<= 17-way); the
// result of an MSM is a canonical group element, so the GPU is free to organise the work
// differently.  Steps 1-4 (the sort) are in msm_sort.hip, built once for both curves; 5-7 (the pass, the reductions, the fold) and
// the window-table builder are here, built once per curve; the host planner (MsmPlan) is msm_plan.hip:
//
//   1. digits_kernel       scalars (Montgomery Fr) -> canonical (prover.rs:63-65 into_bigint)
//                           -> biased signed digits, written as W coalesced u16 "digit planes"
//   2. bucket_count_kernel  per (point-chunk, window) workgroup: LDS-resident bucket histogram
//                           (2^(c-1) counters, <= 128 KiB of the 160 KiB LDS) flushed with one
//                           global atomic per non-empty bucket
//   3. scan_*_kernel, bucket_slots_kernel   prefix sums: bucket offsets, then partial-sum slot offsets
//   4. bucket_scatter_kernel  same LDS histogram, then one global atomic per bucket reserves a
//                           slice and LDS atomics hand out the slots: a counting sort of
//                           (point index | sign) by (window, bucket) -- order inside a bucket is
//                           irrelevant because group addition commutes
//      (1, 2, 4 as written serve ad-hoc bases -- g16_msm_g1 / _g2; proving-key MSMs use the merged-window variants:
//       class_count / class_partition, then sub_count / sub_partition / final_sort (4m) -- no global atomics, workgroups that fit on
//       a compute unit beside the bucket passes; bucket_count_merged / bucket_wg_scan / bucket_scatter_merged serve padded regions)
//   5. bucket_accumulate30_kernel  THE hot kernel: one lane (G1) / lane pair (G2) per 64-entry SEGMENT of the
//                           sorted list gathers affine bases (96 B / 192 B each) and folds them with XYZZ
//                           mixed additions (8M+2S, no inversion; Y3 under one reduction) in 30-bit lazy arithmetic
//                           (fp30.hpp), the running sum's four coordinates parked in LDS (AccParked, round 4),
//                           flushing one partial sum per (bucket, segment) it touches.  ONE launch walks up to four MSMs
//                           (PassBatch, round 5: the G1 MSMs of a proof that are ready together -- one tail instead of four).
//                           The prover's merged-window sorts use the BUCKET-PART walk instead (MsmPlan::walk, part_walk.hpp:
//                           bucket_parts30_kernel here, its task list from the sort's part_count / part_place kernels): one lane (pair)
//                           per part of ONE bucket, at most Lmax entries, tasks ordered by length -- no boundary test and no flush in
//                           the loop, one store at the end
//   5b. heavy_reduce_kernel cooperative combine of the FEW buckets with MANY partial sums (> 16)
//   5c. bucket_combine_kernel (round 5)  every other bucket's partial sums added up by one lane per BUCKET, so that ...
//   6. bucket_reduce_kernel / window_reduce_kernel   ... sum_b (b+1) S_b by chunked running sums reads ONE sum per bucket: a chain
//                           of 2 G dependent additions per lane; chunk offsets through bit-plane sums of the chunk totals
//                           (MsmPlan in internal.hpp), not a scalar multiplication
//   7. host                 recombine the planes per group, then sum_w 2^(cw) R_w  (<= 256 doublings); a bucket-space shard
//                           (MsmPlan::shard_n, round 5: the rank owns the buckets b mod N == rank and indexes them by b / N)
//                           turns its local sums into its share  N sum_k (k+1) S_k - (N - 1 - rank) sum_k S_k
//
// Steps 1-4 depend only on the scalars and are shared by every MSM over the same scalar
// vector (a_query, b_g1_query, b_g2_query and l_query all use the witness: one sort, four
// accumulations).
//
// MERGED WINDOWS (proving-key queries).  The bases of a proving key are fixed, so g16_pk_load precomputes the window
// tables T[j][i] = 2^(cj) P_i (build_window_tables_kernel).  Window j's digit of scalar i then selects T[j][i] and ALL
// windows share one set of 2^(c-1) buckets: sum_i s_i P_i = sum_b (b+1) sum_{(i,j): |d_ij|-1 = b} +-T[j][i].  The bucket
// count no longer grows with the number of windows, so c rises from 16 to 20 and the bucket pass folds n*13 instead
// of n*16 points (BLS12-381 and BN254 scalars); the 2^19 buckets are cut into 64 sort classes of 2^13 for the LDS histogram
// (msm_sort.hip) and into 16 groups of 2^15 for the reductions, which treat a group like a window.  Costs 13x the key's
// memory (31 GB at 2^22 constraints on BLS12-381 -- HBM capacity is what this GPU has to spare) and a one-off table build at load time.
// Roofline: step 5 reads ~N*W*(sizeof(Affine)+4) bytes (6.9 GB measured per MSM at 2^22, G1, merged windows) but spends ~10
// field products (3 169 v_mad_u64_u32) per 100 bytes, i.e. it is integer-VALU bound, not HBM bound; the
// bytes/s it sustains is reported against the 8 TB/s roofline by bench.py regardless.
#include "internal.hpp"
#include "fp30.hpp"
#include "acc_store.hpp"
#include "pass_batch.hpp"
#include "batch_affine.hpp"
#include "window_tables.hpp"
#include <algorithm>
#include <cstdlib>

namespace g16 {

static constexpr int RED_THREADS = 64;
static constexpr int WIN_THREADS = 256;  // lanes of the per-window reduction

// ---------------------------------------------------------------------------------------------
// 5. bucket accumulation (THE hot kernel), 30-bit lazy arithmetic (fp30.hpp); F30 = Fp30<P> (G1) or Fp2p30<P> (G2, lane pair).
// Work unit = a SEGMENT of Lseg consecutive entries of the bucket-sorted list, not a bucket: every lane walks exactly
// Lseg entries, so lanes of a wave finish together whatever the bucket-size distribution (one lane per whole bucket, in bucket
// order, left ~18 % of lane time idle at a mean bucket load of 128, ~35 % at 16: what idled the lanes was the missing order by
// length, which the bucket-part walk has).  When the walk crosses a bucket boundary the running sum
// is flushed -- raw lazy limbs, no conversion -- into that bucket's slot for this segment (slot offsets from the scan),
// so a bucket ends up with one partial sum per segment it touches; the reduction kernels add them up.
// `bases` hold canonical x*R', y*R' packed in 32-bit words (convert_bases30_kernel).
// DIRECT (batched-affine plan): the walk is over the level-R list itself -- slot e holds an affine point (or the identity),
// bucket b owns slots [offsets[b] >> off_shift, offsets[b + 1] >> off_shift) -- instead of over sorted entry words.
// Stores for the reductions' streamed additions (acc_add_streamed, fp30.hpp).
// An AccRaw record in LDS or global memory as the lane(s) of one task see it: coordinate k of a one-lane field is the k-th F30 of the
// record; of the lane pair, component (lane parity) of the k-th Fq2.  Identity <=> zz is all-zero limbs (AccRaw).
template <class F30>
struct RawAccStore {
    AccRaw<typename F30::Raw>* p;
    __device__ __forceinline__ F30 ld(int k) const {
        asm volatile("" ::: "memory");   // a fresh read where it is needed, not a value kept live from the top of the formula
        if constexpr (F30::LANES_PER_TASK == 1) {
            static_assert(sizeof(F30) == sizeof(typename F30::Raw), "one-lane fields share the raw layout");
            return reinterpret_cast<const F30*>(p)[k];
        } else {
            typedef typename F30::B B30;
            return F30{reinterpret_cast<const B30*>(p)[2 * k + (F30::lane_hi() ? 1 : 0)]};
        }
    }
    __device__ __forceinline__ void st(int k, const F30& a) const {
        if constexpr (F30::LANES_PER_TASK == 1) {
            reinterpret_cast<F30*>(p)[k] = a;
        } else {
            typedef typename F30::B B30;
            reinterpret_cast<B30*>(p)[2 * k + (F30::lane_hi() ? 1 : 0)] = a.c;
        }
        asm volatile("" ::: "memory");
    }
    __device__ __forceinline__ bool inf() const {
        const F30 zz = ld(2);
        if constexpr (F30::LANES_PER_TASK == 1) return zz.raw_zero();
        else return F30::both(zz.c.raw_zero());
    }
    __device__ __forceinline__ void set_inf() const { st(2, F30::zero()); }
};
// four coordinates in registers (one-lane fields: the running sum of the bucket reduction)
template <class F30>
struct RegAccStore {
    F30 v[4];
    __device__ __forceinline__ F30 ld(int k) const { return v[k]; }
    __device__ __forceinline__ void st(int k, const F30& a) { v[k] = a; }
};
template <class F30, class St>
__device__ __forceinline__ Acc30<F30> gather_acc(const St& st, bool inf) {
    Acc30<F30> a;
    a.inf = inf;
    if (inf) { a.x = a.y = a.zz = a.zzz = F30::zero(); return a; }
    a.x = st.ld(0); a.y = st.ld(1); a.zz = st.ld(2); a.zzz = st.ld(3);
    return a;
}

// ONE launch walks up to PASS_BATCH MSMs (blockIdx.y = MSM of the batch: its own bases, sorted list, offsets and partial-sum slots; one
// plan).  A pass ends with a tail -- the last segments run on a chip that is emptying: about half a segment's time when the lanes are
// re-filled dynamically -- and a launch's tail cannot be filled by the next launch of the same stream.  The G1 MSMs of a proof that are
// ready together (l, a, b_g1 share the witness sort; h joins when its sort is done in time) therefore go as ONE launch: one tail
// instead of three or four (a rank's share of an 8-way sharded 2^22 proof: 1.3-1.4 ms per pass of 1.1 ms of work, round 5).
// (pass_batch.hpp: PASS_BATCH and PassBatch, shared with bucket_parts30_kernel below)
template <class F30, bool DIRECT>
__global__ __launch_bounds__(ACC_THREADS, F30::ACC_MIN_WAVES) void bucket_accumulate30_kernel(
    PassBatch<F30> batch, uint32_t M, uint32_t off_shift, uint32_t lseg, uint32_t merged) {
    // (uniform index: the seven values come out of the kernel arguments with scalar loads)
    const Affine<typename F30::Std>* __restrict__ bases = batch.bases[blockIdx.y];
    const int64_t shift = batch.shift[blockIdx.y];
    const uint64_t base_count = batch.base_count[blockIdx.y];
    const uint32_t* __restrict__ sorted = batch.sorted[blockIdx.y];
    const uint32_t* __restrict__ offsets = batch.offsets[blockIdx.y];
    const uint32_t* __restrict__ slot_off = batch.slot_off[blockIdx.y];
    AccRaw<typename F30::Raw>* __restrict__ partials = batch.partials[blockIdx.y];
    const uint32_t t = (blockIdx.x * ACC_THREADS + threadIdx.x) / F30::LANES_PER_TASK;   // lanes of one task are adjacent
    const uint32_t S = offsets[M] >> off_shift;                                            // entries in total
    const uint64_t start64 = (uint64_t)t * lseg;
    if (start64 >= S) return;
    const uint32_t start = (uint32_t)start64;
    const uint32_t end = (uint32_t)min((uint64_t)S, start64 + lseg);
    uint32_t lo = 0, hi = M;  // bucket containing `start`: offsets[lo] <= start < offsets[lo + 1]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((offsets[mid] >> off_shift) <= start) lo = mid; else hi = mid;
    }
    uint32_t b = lo, b_first = offsets[b] >> off_shift, b_end = offsets[b + 1] >> off_shift;
    // the running sum's coordinates live in LDS (AccParked)
    __shared__ __attribute__((aligned(16))) uint32_t acc_lds[4 * F30::PREFIX_LIMBS * ACC_THREADS];
    AccParked<F30, LdsAccStore<F30>> acc;
    acc.s.quad = acc_lds + 4 * threadIdx.x;
    acc.s.tail = acc_lds + 4 * LdsAccStore<F30>::QUADS * ACC_THREADS + threadIdx.x;
    acc.inf = true;
    auto flush = [&](AccRaw<typename F30::Raw>* dst) { acc.gather().store_raw(dst); acc.inf = true; };
    // software pipeline: the base point of entry e+1 is gathered (and the sorted word of entry e+2 loaded) before the
    // ~20k-instruction addition of entry e, so the HBM latencies hide under arithmetic.  (Touching the cache lines of
    // entry e+2 with direct-to-LDS loads was tried for the window tables' wider gather: 25 % slower.)
    uint32_t v_next = 0;
    // y stays PACKED (12 words as gathered): the signed digit's negation costs one subtract-with-borrow per word there, and the
    // unpacking happens once, when the point is added (AccParked::add_affine_packed)
    typedef typename F30::PackedC YNext;
    F30 px_next = F30::zero();
    YNext py_next = YNext::zero();
    bool ok_next = false;
    auto decode = [&](uint32_t v, int64_t* at) -> bool {
        // per-window plan: entry = point | sign<<31 ; merged plan: point | window<<26 | sign<<31, base = table[window][point]
        const uint32_t pt = merged ? (v & 0x3ffffffu) : (v & 0x7fffffffu);
        const uint64_t row = merged ? (uint64_t)((v >> 26) & 31u) * base_count : 0;
        const int64_t idx = (int64_t)pt + shift;
        *at = (int64_t)row + idx;
        return idx >= 0 && (uint64_t)idx < base_count;
    };
    auto fetch = [&](uint32_t v) {   // DIRECT: v is the slot index itself
        v_next = DIRECT ? 0u : v;
        int64_t at = (int64_t)v;
        ok_next = DIRECT ? true : decode(v, &at);
        if (ok_next) ok_next = F30::load_point_py(bases, at, px_next, py_next);
    };
    fetch(DIRECT ? start : sorted[start]);
    uint32_t v_fetch = DIRECT ? start + 1 : (start + 1 < end ? sorted[start + 1] : 0u);   // entry e+1's word, loaded one iteration early
    for (uint32_t e = start; e < end; ++e) {
        if (e == b_end) {  // crossed into the next non-empty bucket: flush this segment's share of bucket b
            flush(&partials[slot_off[b] + (t - b_first / lseg)]);
            do { ++b; b_end = offsets[b + 1] >> off_shift; } while (b_end <= e);
            b_first = offsets[b] >> off_shift;
        }
        const uint32_t v = v_next;
        const F30 px = px_next;
        YNext py = py_next;
        const bool ok = ok_next;
        auto advance = [&]() {
            if (e + 1 < end) fetch(v_fetch);
            if constexpr (DIRECT) v_fetch = e + 2;
            else v_fetch = e + 2 < end ? sorted[e + 2] : 0u;
        };
        if constexpr (F30::ACC_PREFETCH) advance();
        if (ok) acc.add_affine_packed(px, py, (v >> 31) != 0);   // the digit's sign and the parked sum's sign are one flip (AccParked)
        if constexpr (!F30::ACC_PREFETCH) advance();
    }
    flush(&partials[slot_off[b] + (t - b_first / lseg)]);
}

// the largest v of the wave, in a scalar register
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    G16_UNROLL for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The bucket pass over PARTS (part_walk.hpp; the segment walk: bucket_accumulate30_kernel above).  Lane (pair) i of MSM blockIdx.y reads
// descriptor i -- the list is ordered by length, so the wave's tasks have one trip count, or two where it straddles two length classes --
// walks its entries with the segment walk's software pipeline (walk_bucket_part) and stores its sum once, into its slot.  No search for
// the first bucket, no boundary test, no flush and no slot arithmetic in the loop; the first entry's set and the final store are uniform
// across the wave.  The grid covers a host upper bound on the slots; slot_off[M] is the real count.  Same launch bounds, same parked
// accumulator and the same LDS as the segment walk's kernel: three waves per SIMD for G1, two for the lane pair.
template <class F30>
__global__ __launch_bounds__(ACC_THREADS, F30::ACC_MIN_WAVES) void bucket_parts30_kernel(PassBatch<F30> batch, PartTaskBatch lists, uint32_t M,
                                                                                         uint32_t merged) {
    const Affine<typename F30::Std>* __restrict__ bases = batch.bases[blockIdx.y];
    const int64_t shift = batch.shift[blockIdx.y];
    const uint64_t base_count = batch.base_count[blockIdx.y];
    const uint32_t* __restrict__ sorted = batch.sorted[blockIdx.y];
    const uint32_t* __restrict__ slot_off = batch.slot_off[blockIdx.y];
    AccRaw<typename F30::Raw>* __restrict__ partials = batch.partials[blockIdx.y];
    const PartTask* __restrict__ tasks = lists.tasks[blockIdx.y];
    const uint32_t t = (blockIdx.x * ACC_THREADS + threadIdx.x) / F30::LANES_PER_TASK;   // lanes of one task are adjacent
    const uint32_t ntasks = slot_off[M];
    PartTask task{0u, 0u, 0u};
    if (t < ntasks) task = tasks[t];
    const uint32_t trip = wave_max_u32(task.len);
    if (t >= ntasks) return;
    __shared__ __attribute__((aligned(16))) uint32_t acc_lds[4 * F30::PREFIX_LIMBS * ACC_THREADS];
    AccParked<F30, LdsAccStore<F30>> acc;
    acc.s.quad = acc_lds + 4 * threadIdx.x;
    acc.s.tail = acc_lds + 4 * LdsAccStore<F30>::QUADS * ACC_THREADS + threadIdx.x;
    acc.inf = true;
    walk_bucket_part<F30>(task, trip, sorted, bases, shift, base_count, merged != 0, acc, &partials[task.slot]);
}

// ---------------------------------------------------------------------------------------------
// 5a. batched-affine tree levels (batch_affine.hpp): one launch per level, AFF_THREADS / 64 waves per workgroup
// ---------------------------------------------------------------------------------------------
static constexpr int AFF_THREADS = 128;
template <class F30, bool LEVEL0>
__global__ __launch_bounds__(AFF_THREADS, 2) void affine_level_kernel(AffineLevelArgs<F30> args) {
    const uint32_t wave = (blockIdx.x * AFF_THREADS + threadIdx.x) >> 6;
    AffineLevel<F30, LEVEL0>::run(args, wave, threadIdx.x & 63u);
}

template <class P> G16_HD Fp<P> to_r30(const Fp<P>& x) { return Fp30<P>::std_to_r30(x); }
template <class P> G16_HD Fp2<P> to_r30(const Fp2<P>& x) { return {Fp30<P>::std_to_r30(x.c0), Fp30<P>::std_to_r30(x.c1)}; }

template <class F>
__global__ void convert_bases30_kernel(Affine<F>* __restrict__ pts, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> a = pts[i];
    a.x = to_r30(a.x);  // 0 stays 0: the identity encoding (0, 0) is preserved
    a.y = to_r30(a.y);
    pts[i] = a;
}

// field used by the bucket pass and the reduction kernels: Fq as it is; Fq2 on lane pairs (two lanes per bucket, one component each) --
// no scratch, each dependent group operation ~1.7x shorter than one lane per task, and what bounds a rank's share of a sharded proof
// is the G2 reduction chain (the one-lane Fq2 forms: DESIGN.md "Tried and retired")
template <class F> struct Lazy30;
template <class P> struct Lazy30<Fp<P>> { typedef Fp30<P> type; };
template <class P> struct Lazy30<Fp2<P>> { typedef Fp2p30<P> type; };

// ---------------------------------------------------------------------------------------------
// 5b. heavy buckets: a bucket with many partial sums (short top window, repeated scalars such as the all-equal
//     witness of benches/bench.rs:52-54, a boolean witness, ...) has them combined cooperatively by one workgroup; the
//     result replaces the bucket's first partial (the bucket reduction reads only that one for such buckets).
// ---------------------------------------------------------------------------------------------
static constexpr int HEAVY_THREADS = 128;
// Waves per SIMD the one-lane (G1) first-stage reduction kernels are compiled for.  -DG16_FIRST_STAGE_WAVES=4 holds them to 128 registers
// (92 - 112 B of scratch per lane on BLS12-381) so that one of their waves fits BESIDE two G1-pass waves and the stage runs underneath
// the next pass instead of waiting for its workgroups to retire -- measured and lost (round 5, same box, profiles/
// r05_ab_first_stage_128_registers.txt): 65.88 / 65.89 vs 65.57 / 65.52 ms per proof, 8-way share 10.85 / 10.88 vs 10.62 / 10.60 ms.
// The stage is off the critical path either way; co-resident it takes issue slots from the pass and pays for its spills.
#ifndef G16_FIRST_STAGE_WAVES
#define G16_FIRST_STAGE_WAVES 2
#endif
static constexpr int HEAVY_BLOCKS = 512;

// The reductions of up to REDUCE_BATCH MSMs run as ONE launch each (blockIdx.y / .z = MSM of the batch): a reduction is a chain of
// dependent additions in a few hundred waves, so one MSM's reduction alone leaves most of the chip idle, and run underneath the next
// MSM's bucket pass it takes register slots from it for milliseconds (8-way shard at 2^22: 1.8-2.1 ms per pass instead of 1.2).
// The prover therefore runs its four G1 bucket passes back to back and reduces them together.  All MSMs of a batch share the plan
// (bucket count, chunking); slot offsets / heavy lists are per MSM (h has its own sort).
static constexpr int REDUCE_BATCH = 4;
template <class Raw, class X>
struct ReduceBatch {
    Raw* partials[REDUCE_BATCH];
    const uint32_t* slot_off[REDUCE_BATCH];
    const uint32_t* heavy[REDUCE_BATCH];
    Raw* chunk_out[REDUCE_BATCH];       // weighted chunk sums, then (at + chunks) the plain chunk sums
    X* window_sums[REDUCE_BATCH];
};

// (task = one lane, or one lane pair for the lane-pair Fq2: both lanes of a pair run the same control flow)
template <class F30>
__global__ __launch_bounds__(HEAVY_THREADS, F30::LANES_PER_TASK == 1 ? G16_FIRST_STAGE_WAVES : 2) void heavy_reduce_kernel(ReduceBatch<AccRaw<typename F30::Raw>, XYZZ<typename F30::Std>> batch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    AccRaw<typename F30::Raw>* sh = reinterpret_cast<AccRaw<typename F30::Raw>*>(smem);
    constexpr uint32_t LPT = F30::LANES_PER_TASK, TASKS = HEAVY_THREADS / LPT;
    AccRaw<typename F30::Raw>* __restrict__ partials = batch.partials[blockIdx.y];
    const uint32_t* __restrict__ slot_off = batch.slot_off[blockIdx.y];
    const uint32_t* __restrict__ heavy = batch.heavy[blockIdx.y];
    const uint32_t nheavy = heavy[0], task = threadIdx.x / LPT;
    for (uint32_t i = blockIdx.x; i < nheavy; i += gridDim.x) {
        const uint32_t b = heavy[1 + i];
        const uint32_t t0 = slot_off[b], t1 = slot_off[b + 1];
        // streamed additions (acc_add_streamed): the task's sum lives in its LDS record from the start, every operand
        // coordinate is fetched where it is consumed -- no 8-coordinate operand pair in registers
        __syncthreads();  // previous iteration's readers are done with sh / partials[t0]
        const RawAccStore<F30> mine{&sh[task]};
        bool inf = true;
        for (uint32_t q = t0 + task; q < t1; q += TASKS) {
            const RawAccStore<F30> src{&partials[q]};
            acc_add_streamed<F30>(mine, inf, src, src.inf());
        }
        if (inf) mine.set_inf();
        __syncthreads();
        for (uint32_t d = TASKS / 2; d > 0; d >>= 1) {
            if (task < d) {
                const RawAccStore<F30> other{&sh[task + d]};
                bool mi = mine.inf();
                const bool was = mi;
                acc_add_streamed<F30>(mine, mi, other, other.inf());
                if (mi && !was) mine.set_inf();
            }
            __syncthreads();
        }
        if (task == 0) Acc30<F30>::load_raw(sh[0]).store_raw(&partials[t0]);
    }
}

// ---------------------------------------------------------------------------------------------
// 5c. every other bucket with more than one partial sum (2 .. HEAVY_PARTS of them): ONE task per BUCKET adds them up into the bucket's
//     first slot, so that the bucket reduction below -- one lane per G buckets, a chain of dependent additions whose length IS the time
//     it takes (a lone wave issues a dependent instruction every ~7.5 cycles: ~27 us per G1 addition) -- reads one sum per bucket:
//     G (np + 1) additions per lane become (np - 1) here, spread over G times the lanes, and 2 G there.  Round 5: the reductions are
//     what a rank's share of a sharded proof ends with (8-way at 2^22: 1.0 ms -> 0.45 ms of bucket level per G1 batch), and the G2
//     reduction runs its chain underneath the G1 passes.
// ---------------------------------------------------------------------------------------------
template <class F30>
__global__ __launch_bounds__(RED_THREADS, F30::LANES_PER_TASK == 1 ? G16_FIRST_STAGE_WAVES : 2) void bucket_combine_kernel(ReduceBatch<AccRaw<typename F30::Raw>, XYZZ<typename F30::Std>> batch, uint32_t M) {
    AccRaw<typename F30::Raw>* __restrict__ partials = batch.partials[blockIdx.y];
    const uint32_t* __restrict__ slot_off = batch.slot_off[blockIdx.y];
    const uint32_t b = (blockIdx.x * RED_THREADS + threadIdx.x) / F30::LANES_PER_TASK;   // lanes of one task are adjacent
    if (b >= M) return;
    const uint32_t t0 = slot_off[b], np = slot_off[b + 1] - t0;
    if (np < 2 || np > HEAVY_PARTS) return;   // (heavy buckets were combined into [t0] by heavy_reduce_kernel)
    const RawAccStore<F30> mine{&partials[t0]};
    bool inf = mine.inf();
    for (uint32_t q = 1; q < np; ++q) {
        const RawAccStore<F30> src{&partials[t0 + q]};
        acc_add_streamed<F30>(mine, inf, src, src.inf());
    }
    // Several additions into one slot: an identity first partial may have been overwritten by a point that a later partial cancelled
    // ([O, P, -P]), which leaves the flag set and P's zz in the record -- so the identity is written whenever the flag ends set, not
    // only when the slot held a point at the start.  (The trees of heavy_reduce_kernel / window_reduce_kernel add once per step.)
    if (inf) mine.set_inf();
}

// ---------------------------------------------------------------------------------------------
// 6. bucket reduction: chunk of G buckets per lane, then one workgroup per window
// ---------------------------------------------------------------------------------------------
template <class F30>
__global__ __launch_bounds__(RED_THREADS, 2) void bucket_reduce_kernel(ReduceBatch<AccRaw<typename F30::Raw>, XYZZ<typename F30::Std>> batch, uint32_t B, int W,
                                                                    uint32_t G) {
    const AccRaw<typename F30::Raw>* __restrict__ partials = batch.partials[blockIdx.y];
    const uint32_t* __restrict__ slot_off = batch.slot_off[blockIdx.y];
    const uint32_t cpw = B / G;
    AccRaw<typename F30::Raw>* __restrict__ chunk_out = batch.chunk_out[blockIdx.y];
    AccRaw<typename F30::Raw>* __restrict__ chunk_sum = chunk_out + (size_t)cpw * W;
    const uint32_t t = (blockIdx.x * RED_THREADS + threadIdx.x) / F30::LANES_PER_TASK;   // lanes of one task are adjacent
    if (t >= cpw * (uint32_t)W) return;
    const uint32_t w = t / cpw, ch = t % cpw, b_lo = ch * G;
    // two running sums, `run` (the buckets so far) and `tot` (the runs), added to with acc_add_streamed: the partial sums come
    // straight from their records in memory, `tot` lives in LDS, and `run` in LDS too for the lane pair (for the one-lane field it
    // stays in registers: 13 KB of LDS per workgroup keeps eight workgroups per CU for the batched G1 reduction of the tail)
    constexpr bool PAIR = F30::LANES_PER_TASK == 2;
    constexpr int SLOTS = PAIR ? 8 : 4;
    __shared__ __attribute__((aligned(16))) uint32_t red_lds[SLOTS * F30::PREFIX_LIMBS * RED_THREADS];
    static_assert(RED_THREADS == ACC_THREADS, "LdsAccStore is laid out for ACC_THREADS lanes");
    LdsAccStore<F30> tot_s;
    tot_s.quad = red_lds + 4 * threadIdx.x;
    tot_s.tail = red_lds + 4 * LdsAccStore<F30>::QUADS * RED_THREADS + threadIdx.x;
    typename std::conditional<PAIR, LdsAccStore<F30>, RegAccStore<F30>>::type run_s;
    if constexpr (PAIR) {
        run_s.quad = tot_s.quad + 4 * LdsAccStore<F30>::WORDS_PER_VALUE;
        run_s.tail = tot_s.tail + 4 * LdsAccStore<F30>::WORDS_PER_VALUE;
    }
    bool run_inf = true, tot_inf = true;
    for (uint32_t bb = G; bb-- > 0;) {
        const uint32_t gb = w * B + b_lo + bb;
        const uint32_t t0 = slot_off[gb];
        if (slot_off[gb + 1] != t0) {   // the bucket's partial sums were combined into [t0] (heavy_reduce_kernel / bucket_combine_kernel)
            const RawAccStore<F30> src{const_cast<AccRaw<typename F30::Raw>*>(&partials[t0])};
            acc_add_streamed<F30>(run_s, run_inf, src, src.inf());
        }
        acc_add_streamed<F30>(tot_s, tot_inf, run_s, run_inf);
    }
    // sum_b (b+1) S_b over the chunk = tot + b_lo * run: the b_lo * run part is assembled from bit-plane sums of `run` over
    // the chunks by the window level and the host (MsmPlan) -- no scalar multiplication in this chain of dependent additions
    gather_acc<F30>(run_s, run_inf).store_raw(&chunk_sum[t]);
    gather_acc<F30>(tot_s, tot_inf).store_raw(&chunk_out[t]);
}

// grid = (groups, planes): plane 0 sums the chunks' weighted sums, plane 1 their plain sums, plane 2 + k the plain sums of the
// chunks whose index has bit k set
template <class F30>
__global__ __launch_bounds__(WIN_THREADS, 2) void window_reduce_kernel(ReduceBatch<AccRaw<typename F30::Raw>, XYZZ<typename F30::Std>> batch, uint32_t cpw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    AccRaw<typename F30::Raw>* sh = reinterpret_cast<AccRaw<typename F30::Raw>*>(smem);
    constexpr uint32_t LPT = F30::LANES_PER_TASK, TASKS = WIN_THREADS / LPT;
    const uint32_t w = blockIdx.x, p = blockIdx.y, task = threadIdx.x / LPT;
    const AccRaw<typename F30::Raw>* __restrict__ chunk_out = batch.chunk_out[blockIdx.z];
    const AccRaw<typename F30::Raw>* __restrict__ chunk_sum = chunk_out + (size_t)cpw * gridDim.x;
    XYZZ<typename F30::Std>* __restrict__ window_sums = batch.window_sums[blockIdx.z];
    const AccRaw<typename F30::Raw>* src = (p == 0 ? chunk_out : chunk_sum) + (uint64_t)w * cpw;
    const uint32_t mask = p >= 2 ? 1u << (p - 2) : 0u;
    // streamed additions, as in heavy_reduce_kernel
    const RawAccStore<F30> mine{&sh[task]};
    bool inf = true;
    for (uint32_t j = task; j < cpw; j += TASKS)
        if (!mask || (j & mask)) {
            const RawAccStore<F30> s_j{const_cast<AccRaw<typename F30::Raw>*>(&src[j])};
            acc_add_streamed<F30>(mine, inf, s_j, s_j.inf());
        }
    if (inf) mine.set_inf();
    __syncthreads();
    for (uint32_t d = TASKS / 2; d > 0; d >>= 1) {
        if (task < d) {
            const RawAccStore<F30> other{&sh[task + d]};
            bool mi = mine.inf();
            const bool was = mi;
            acc_add_streamed<F30>(mine, mi, other, other.inf());
            if (mi && !was) mine.set_inf();
        }
        __syncthreads();
    }
    // the plane sums are what leaves the device: standard arkworks Montgomery radix
    if (task == 0) Acc30<F30>::load_raw(sh[0]).store_std(&window_sums[(uint64_t)w * gridDim.y + p]);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// buffers of one MSM's pass and reductions
template <class F>
static int alloc_msm_buffers(const ScalarSort& ss, Arena& arena, MsmBuffers<F>* out) {
    typedef AccRaw<typename Lazy30<F>::type::Raw> Raw;
    const MsmPlan& plan = ss.plan;
    const uint32_t cpw = plan.B / plan.chunk_buckets();
    Raw *partials = nullptr, *chunk_out = nullptr;
    G16_TRY(arena.alloc_n((size_t)ss.max_tasks ? ss.max_tasks : 1, &partials));
    G16_TRY(arena.alloc_n((size_t)cpw * plan.groups * 2, &chunk_out));   // weighted chunk sums, then plain chunk sums
    G16_TRY(arena.alloc_n((size_t)plan.outputs(), &out->window_sums));
    out->partials = partials;
    out->chunk_out = chunk_out;
    return G16_OK;
}

template <class F>
int msm_bucket_pass(const Affine<F>* d_bases, int64_t shift, uint64_t base_count, const ScalarSort& ss, Arena& arena, hipStream_t st,
                    MsmBuffers<F>* out, EventTimer* bucket_timer) {
    typedef typename Lazy30<F>::type F30;
    typedef AccRaw<typename Lazy30<F>::type::Raw> Raw;
    const MsmPlan& plan = ss.plan;
    const uint32_t M = plan.buckets();
    const int R = plan.affine_levels;
    if (!R || !ss.max_sorted) {
        const PassJob<F> job{d_bases, shift, base_count, &ss, out};
        return msm_bucket_pass_batch<F>(&job, 1, arena, st, bucket_timer);
    }
    G16_TRY(alloc_msm_buffers<F>(ss, arena, out));
    Raw* partials = static_cast<Raw*>(out->partials);
    // batched-affine levels: two ping-pong lists (level 1 holds max_sorted / 2 points, level 2 a quarter, level 3 reuses the
    // first, ...) and the prefix-product scratch of the widest level
    Affine<F>* lists[2] = {nullptr, nullptr};
    Word4* prefix = nullptr;
    constexpr uint32_t T = 64 / F30::LANES_PER_TASK;
    constexpr int QUADS = AffineLevel<F30, true>::QUADS;
    auto level_K = [&](int r) -> uint32_t {   // steps per task: as many as keep >= ~2 k waves in flight, 8 .. 64
        const uint64_t pairs = ss.max_sorted >> (r + 1);
        uint32_t K = 64;
        while (K > 8 && pairs / ((uint64_t)K * T) < 2048) K >>= 1;
        return K;
    };
    auto level_waves = [&](int r) -> uint64_t { return ((ss.max_sorted >> (r + 1)) + (uint64_t)level_K(r) * T - 1) / ((uint64_t)level_K(r) * T); };
    {
        G16_TRY(arena.alloc_n((size_t)(ss.max_sorted >> 1) + 1, &lists[0]));
        if (R > 1) G16_TRY(arena.alloc_n((size_t)(ss.max_sorted >> 2) + 1, &lists[1]));
        size_t recs = 0;
        for (int r = 0; r < R; ++r) recs = std::max(recs, (size_t)(level_waves(r) * level_K(r)) * QUADS * 64);
        G16_TRY(arena.alloc_n(recs ? recs : 1, &prefix));
    }
    if (bucket_timer) G16_TRY(bucket_timer->start(st));
    {
        AffineLevelArgs<F30> a;
        a.sorted = ss.sorted;
        a.total = ss.offsets + M;
        a.prefix = prefix;
        a.shift = shift;
        a.base_count = base_count;
        a.merged = plan.merged ? 1u : 0u;
        for (int r = 0; r < R; ++r) {
            a.in = r == 0 ? d_bases : lists[(r - 1) & 1];
            a.out = lists[r & 1];
            a.level = (uint32_t)r;
            a.K = level_K(r);
            const uint64_t waves = level_waves(r);
            const unsigned blocks = (unsigned)((waves * 64 + AFF_THREADS - 1) / AFF_THREADS);
            if (r == 0) hipLaunchKernelGGL((affine_level_kernel<F30, true>), dim3(blocks), dim3(AFF_THREADS), 0, st, a);
            else hipLaunchKernelGGL((affine_level_kernel<F30, false>), dim3(blocks), dim3(AFF_THREADS), 0, st, a);
            G16_LAUNCH_CHECK();
        }
    }
    if (ss.max_segments) {
        const uint64_t lanes = (uint64_t)ss.max_segments * F30::LANES_PER_TASK;
        const dim3 grid((unsigned)((lanes + ACC_THREADS - 1) / ACC_THREADS));
        PassBatch<F30> b;
        for (int i = 0; i < PASS_BATCH; ++i) {
            b.bases[i] = lists[(R - 1) & 1]; b.shift[i] = 0; b.base_count[i] = 0; b.sorted[i] = nullptr;
            b.offsets[i] = ss.offsets; b.slot_off[i] = ss.task_off; b.partials[i] = partials;
        }
        hipLaunchKernelGGL((bucket_accumulate30_kernel<F30, true>), grid, dim3(ACC_THREADS), 0, st, b, M, (uint32_t)R, plan.Lmax, 0u);
        G16_LAUNCH_CHECK();
    }
    if (bucket_timer) G16_TRY(bucket_timer->stop(st));
    return G16_OK;
}

// Workgroups of the bucket pass per compute unit.  Since round 6 (product-scanning field products: no 2 NL-column array) the G1 kernel
// needs ~140 registers and THREE waves per SIMD fit; what is co-resident is then decided by LDS: 13 312 B of parked accumulator per
// 64-lane workgroup + this pad (unused dynamic LDS).  G16_PASS_WG_PER_CU=n pads so that exactly n workgroups fit (A/B knob).
template <class F30>
static unsigned pass_lds_pad() {
    static const int want = [] { const char* e = getenv("G16_PASS_WG_PER_CU"); return e ? atoi(e) : 0; }();
    if (want <= 0) return 0;
    const unsigned own = 4u * F30::PREFIX_LIMBS * ACC_THREADS * 4u;
    const unsigned per = (160u * 1024u / (unsigned)want) & ~255u;
    return per > own ? per - own : 0;
}

// bucket_parts30_kernel over a host upper bound of `max_tasks` tasks per MSM for the n MSMs of the batch (slot_off[M] is the real count,
// read on the device; surplus lanes exit)
template <class F30>
static int msm_parts_pass_launch(const PassBatch<F30>& batch, const PartTaskBatch& tasks, int n, uint32_t max_tasks, uint32_t M, bool merged,
                                 hipStream_t st) {
    if (n < 1 || n > PASS_BATCH || !max_tasks) return G16_ERR_INTERNAL;
    for (int i = 0; i < n; ++i)
        if (!tasks.tasks[i] || !batch.slot_off[i] || !batch.partials[i]) return G16_ERR_INTERNAL;
    const uint64_t lanes = (uint64_t)max_tasks * F30::LANES_PER_TASK;
    const dim3 grid((unsigned)((lanes + ACC_THREADS - 1) / ACC_THREADS), (unsigned)n);
    hipLaunchKernelGGL((bucket_parts30_kernel<F30>), grid, dim3(ACC_THREADS), pass_lds_pad<F30>(), st, batch, tasks, M, merged ? 1u : 0u);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

// the bucket passes of n <= PASS_BATCH MSMs with one bucket layout as ONE launch (PassBatch above)
template <class F>
int msm_bucket_pass_batch(const PassJob<F>* jobs, int n, Arena& arena, hipStream_t st, EventTimer* bucket_timer) {
    typedef typename Lazy30<F>::type F30;
    typedef AccRaw<typename Lazy30<F>::type::Raw> Raw;
    if (n < 1 || n > PASS_BATCH) return G16_ERR_INTERNAL;
    const MsmPlan& plan = jobs[0].ss->plan;
    for (int i = 0; i < n; ++i) {
        const MsmPlan& q = jobs[i].ss->plan;
        if (q.B != plan.B || q.groups != plan.groups || q.Lmax != plan.Lmax || q.merged != plan.merged || q.walk != plan.walk) return G16_ERR_INTERNAL;
        if (q.walk == MSM_WALK_PARTS && (!jobs[i].ss->tasks || q.affine_levels)) return G16_ERR_INTERNAL;
        if (q.affine_levels && jobs[i].ss->max_sorted) return G16_ERR_INTERNAL;   // that plan walks level lists: msm_bucket_pass
    }
    PassBatch<F30> b;
    PartTaskBatch tb;
    uint32_t max_segments = 0;
    for (int i = 0; i < n; ++i) G16_TRY(alloc_msm_buffers<F>(*jobs[i].ss, arena, jobs[i].out));
    for (int i = 0; i < PASS_BATCH; ++i) {
        const PassJob<F>& j = jobs[i < n ? i : 0];
        b.bases[i] = j.bases; b.shift[i] = j.shift; b.base_count[i] = j.base_count; b.sorted[i] = j.ss->sorted;
        b.offsets[i] = j.ss->offsets; b.slot_off[i] = j.ss->task_off; b.partials[i] = static_cast<Raw*>(j.out->partials);
        tb.tasks[i] = j.ss->tasks;
        if (i < n) max_segments = std::max(max_segments, j.ss->max_segments);
    }
    if (bucket_timer) G16_TRY(bucket_timer->start(st));
    if (max_segments && plan.walk == MSM_WALK_PARTS) {   // max_segments bounds the parts here
        G16_TRY((msm_parts_pass_launch<F30>(b, tb, n, max_segments, plan.buckets(), plan.merged, st)));
    } else if (max_segments) {
        const uint64_t lanes = (uint64_t)max_segments * F30::LANES_PER_TASK;
        const dim3 grid((unsigned)((lanes + ACC_THREADS - 1) / ACC_THREADS), (unsigned)n);
        hipLaunchKernelGGL((bucket_accumulate30_kernel<F30, false>), grid, dim3(ACC_THREADS), pass_lds_pad<F30>(), st, b, plan.buckets(), 0u,
                           plan.Lmax, plan.merged ? 1u : 0u);
        G16_LAUNCH_CHECK();
    }
    if (bucket_timer) G16_TRY(bucket_timer->stop(st));
    return G16_OK;
}

template <class F>
static int reduce_setup(size_t* lds_heavy, size_t* lds_win) {
    typedef typename Lazy30<F>::type F30;
    typedef AccRaw<typename F30::Raw> Raw;
    static PerDeviceOnce attr_once;
    std::atomic<bool>& attr_set = attr_once.flag();
    *lds_heavy = sizeof(Raw) * HEAVY_THREADS / F30::LANES_PER_TASK;
    *lds_win = sizeof(Raw) * WIN_THREADS / F30::LANES_PER_TASK;
    if (!attr_set) {
        G16_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&heavy_reduce_kernel<F30>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)*lds_heavy));
        G16_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&window_reduce_kernel<F30>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)*lds_win));
        attr_set = true;
    }
    return G16_OK;
}

template <class F>
static ReduceBatch<AccRaw<typename Lazy30<F>::type::Raw>, XYZZ<F>> make_reduce_batch(const MsmBuffers<F>* const* bufs, const ScalarSort* const* sorts, int n) {
    typedef AccRaw<typename Lazy30<F>::type::Raw> Raw;
    ReduceBatch<Raw, XYZZ<F>> batch;
    for (int i = 0; i < REDUCE_BATCH; ++i) {
        const int k = i < n ? i : 0;
        batch.partials[i] = static_cast<Raw*>(bufs[k]->partials);
        batch.slot_off[i] = sorts[k]->task_off;
        batch.heavy[i] = sorts[k]->heavy;
        batch.chunk_out[i] = static_cast<Raw*>(bufs[k]->chunk_out);
        batch.window_sums[i] = bufs[k]->window_sums;
    }
    return batch;
}

// the cooperative combine of one MSM's heavy buckets alone (a few hundred workgroups at most: cheap enough to run underneath
// the next bucket pass, which takes it off the batched reduction's chain)
// (n MSMs with one bucket layout: one launch per kernel)
template <class F>
int msm_heavy_reduce_batch(const MsmBuffers<F>* const* bufs, const ScalarSort* const* sorts, int n, hipStream_t st) {
    typedef typename Lazy30<F>::type F30;
    if (n < 1 || n > REDUCE_BATCH) return G16_ERR_INTERNAL;
    const MsmPlan& plan = sorts[0]->plan;
    for (int i = 1; i < n; ++i)
        if (sorts[i]->plan.B != plan.B || sorts[i]->plan.groups != plan.groups) return G16_ERR_INTERNAL;
    size_t lds_heavy, lds_win;
    G16_TRY(reduce_setup<F>(&lds_heavy, &lds_win));
    const auto batch = make_reduce_batch<F>(bufs, sorts, n);
    hipLaunchKernelGGL((heavy_reduce_kernel<F30>), dim3(HEAVY_BLOCKS, n), dim3(HEAVY_THREADS), lds_heavy, st, batch);
    G16_LAUNCH_CHECK();
    const uint32_t M = plan.buckets();
    hipLaunchKernelGGL((bucket_combine_kernel<F30>), dim3((M * F30::LANES_PER_TASK + RED_THREADS - 1) / RED_THREADS, n), dim3(RED_THREADS), 0, st, batch, M);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

template <class F>
int msm_heavy_reduce(const MsmBuffers<F>& buf, const ScalarSort& ss, hipStream_t st) {
    const MsmBuffers<F>* b = &buf;
    const ScalarSort* s = &ss;
    return msm_heavy_reduce_batch<F>(&b, &s, 1, st);
}

template <class F>
int msm_reduce_batch(const MsmBuffers<F>* const* bufs, const ScalarSort* const* sorts, int n, hipStream_t st, bool heavy_done) {
    typedef typename Lazy30<F>::type F30;
    if (n < 1 || n > REDUCE_BATCH) return G16_ERR_INTERNAL;
    const MsmPlan& plan = sorts[0]->plan;
    for (int i = 1; i < n; ++i)
        if (sorts[i]->plan.B != plan.B || sorts[i]->plan.groups != plan.groups) return G16_ERR_INTERNAL;   // one launch = one plan
    const uint32_t G = plan.chunk_buckets();
    const uint32_t cpw = plan.B / G;
    size_t lds_heavy, lds_win;
    G16_TRY(reduce_setup<F>(&lds_heavy, &lds_win));
    const auto batch = make_reduce_batch<F>(bufs, sorts, n);
    if (!heavy_done) G16_TRY((msm_heavy_reduce_batch<F>(bufs, sorts, n, st)));
    hipLaunchKernelGGL((bucket_reduce_kernel<F30>), dim3((cpw * plan.groups * F30::LANES_PER_TASK + RED_THREADS - 1) / RED_THREADS, n), dim3(RED_THREADS), 0,
                       st, batch, plan.B, plan.groups, G);
    G16_LAUNCH_CHECK();
    hipLaunchKernelGGL((window_reduce_kernel<F30>), dim3(plan.groups, plan.planes(), n), dim3(WIN_THREADS), lds_win, st, batch, cpw);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

template <class F>
int msm_reduce(const MsmBuffers<F>& buf, const ScalarSort& ss, hipStream_t st) {
    const MsmBuffers<F>* b = &buf;
    const ScalarSort* s = &ss;
    return msm_reduce_batch<F>(&b, &s, 1, st, false);
}

template <class F>
int convert_bases(Affine<F>* d_bases, uint64_t n, hipStream_t st) {
    if (n == 0) return G16_OK;
    hipLaunchKernelGGL((convert_bases30_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_bases, n);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

template <class F>
XYZZ<F> fold_windows(const XYZZ<F>* ws, const MsmPlan& plan) {
    const int NP = plan.planes(), bits = plan.chunk_bits();
    // per group: T = sum_b (b+1) S_b = P_0 + G * sum_k 2^k P_(2+k)
    auto group_T = [&](int g) -> XYZZ<F> {
        const XYZZ<F>* P = ws + (size_t)g * NP;
        XYZZ<F> hi = XYZZ<F>::identity();
        for (int k = bits - 1; k >= 0; --k) { hi = hi.dbl(); hi.add(P[2 + k]); }
        for (uint32_t b = plan.chunk_buckets(); b > 1; b >>= 1) hi = hi.dbl();
        hi.add(P[0]);
        return hi;
    };
    XYZZ<F> total = XYZZ<F>::identity();
    if (plan.merged) {
        // bucket value of (group q, bucket b) is q*B + b + 1:  sum = sum_q T_q + B * sum_q q S_q
        const int Q = plan.groups;
        if (Q > 1) {
            XYZZ<F> run = XYZZ<F>::identity();
            for (int q = Q - 1; q >= 1; --q) { run.add(ws[(size_t)q * NP + 1]); total.add(run); }
            for (uint32_t b = plan.B; b > 1; b >>= 1) total = total.dbl();
        }
        for (int q = 0; q < Q; ++q) total.add(group_T(q));
        if (plan.shard_n > 1) {
            // bucket-space shard: `total` is sum_k (k+1) S_k over the LOCAL indices; the rank's buckets are b = shard_n k + shard_r, so its
            // share of the MSM is  shard_n * total - (shard_n - 1 - shard_r) * sum_k S_k   (two multiplications by numbers below 64)
            XYZZ<F> plain = XYZZ<F>::identity();
            for (int q = 0; q < Q; ++q) plain.add(ws[(size_t)q * NP + 1]);
            const uint32_t kn = (uint32_t)plan.shard_n, km = (uint32_t)(plan.shard_n - 1 - plan.shard_r);
            total = total.mul_bits(&kn, 7);
            if (km) total.add(plain.mul_bits(&km, 7).neg());
        }
        return total;
    }
    for (int w = plan.W - 1; w >= 0; --w) {
        for (int k = 0; k < plan.c; ++k) total = total.dbl();
        total.add(group_T(w));
    }
    return total;
}

// table[j * n + i] = 2^(c j) P_i (window_tables.hpp): one lane (G1) or one lane pair (G2) per point in the 30-bit lazy arithmetic,
// Jacobian doublings, ONE field inversion per point; the rows' (X, Y, Z, prefix product) wait for the backward sweep in `park`,
// a limb-planar HBM buffer of 4 (W - 1) NL words per lane.  Runs once per key, in chunks of TABLE_CHUNK points.
static constexpr int TABLE_MAX_W = 32;
static constexpr int TABLE_THREADS = 128;
static constexpr uint64_t TABLE_CHUNK = (uint64_t)1 << 18;   // points per launch: 2^18 (G1) / 2^19 (G2) lanes, park <= 1.3 GB
template <class F30>
__global__ __launch_bounds__(TABLE_THREADS, 2) void build_window_tables_kernel(const Affine<typename F30::Std>* __restrict__ src, uint64_t first,
                                                                              uint64_t count, uint64_t n, int c, int W,
                                                                              Affine<typename F30::Std>* __restrict__ table, uint32_t* __restrict__ park) {
    typedef TableDeviceIO<F30> IO;
    typedef typename IO::W32 W32;
    const uint64_t lane = (uint64_t)blockIdx.x * TABLE_THREADS + threadIdx.x;
    const uint64_t t = lane / F30::LANES_PER_TASK;   // lanes of one task are adjacent
    if (t >= count) return;
    const uint64_t i = first + t;
    IO io{reinterpret_cast<const W32*>(src + i), reinterpret_cast<W32*>(table + i), n * 2 * IO::TL::PARTS, park + lane, count * F30::LANES_PER_TASK};
    window_table_task<F30>(io, c, W);
}

template <class F>
size_t window_table_park_bytes(uint64_t n, int W) {
    typedef typename Lazy30<F>::type F30;
    const uint64_t chunk = std::min(n ? n : 1, TABLE_CHUNK);
    return (size_t)4 * (W > 1 ? W - 1 : 1) * TableLane<F30>::B::NL * chunk * F30::LANES_PER_TASK * sizeof(uint32_t);
}

// park: window_table_park_bytes<F>(n, W) of device scratch the caller keeps alive until the stream has run the launches (then
// nothing here waits for the GPU: g16_pk_load queues the builds of all five queries behind one another and allocates the next
// table while the previous one is being built); nullptr: allocated here, and the call returns with the table finished.
template <class F>
int build_window_tables(const Affine<F>* d_src, uint64_t n, int c, int W, Affine<F>* d_table, hipStream_t st, void* park_buf) {
    typedef typename Lazy30<F>::type F30;
    static_assert(sizeof(Affine<F>) == 2 * TableLane<F30>::PARTS * sizeof(typename TableLane<F30>::B::Std), "affine point = x parts | y parts");
    if (n == 0) return G16_OK;
    if (W > TABLE_MAX_W) return G16_ERR_INTERNAL;
    const uint64_t chunk = std::min(n, TABLE_CHUNK);
    uint32_t* park = static_cast<uint32_t*>(park_buf);
    if (!park && hipMalloc((void**)&park, window_table_park_bytes<F>(n, W)) != hipSuccess) { (void)hipGetLastError(); return G16_ERR_OOM; }
    int rc = G16_OK;
    for (uint64_t first = 0; first < n && rc == G16_OK; first += chunk) {
        const uint64_t count = std::min(chunk, n - first);
        const uint64_t lanes = count * F30::LANES_PER_TASK;
        hipLaunchKernelGGL((build_window_tables_kernel<F30>), dim3((unsigned)((lanes + TABLE_THREADS - 1) / TABLE_THREADS)), dim3(TABLE_THREADS), 0, st,
                           d_src, first, count, n, c, W, d_table, park);
        if (hipGetLastError() != hipSuccess) rc = G16_ERR_HIP;
    }
    if (!park_buf) {
        if (hipStreamSynchronize(st) != hipSuccess && rc == G16_OK) rc = G16_ERR_HIP;
        (void)hipFree(park);
    }
    return rc;
}

#define G16_INSTANTIATE_MSM(C)                                                                                               \
    template int convert_bases<typename C::Fq>(Affine<typename C::Fq>*, uint64_t, hipStream_t);                             \
    template int convert_bases<typename C::Fq2>(Affine<typename C::Fq2>*, uint64_t, hipStream_t);                           \
    template int build_window_tables<typename C::Fq>(const Affine<typename C::Fq>*, uint64_t, int, int, Affine<typename C::Fq>*, hipStream_t, void*);    \
    template int build_window_tables<typename C::Fq2>(const Affine<typename C::Fq2>*, uint64_t, int, int, Affine<typename C::Fq2>*, hipStream_t, void*); \
    template size_t window_table_park_bytes<typename C::Fq>(uint64_t, int);                                                 \
    template size_t window_table_park_bytes<typename C::Fq2>(uint64_t, int);                                                \
    template int msm_bucket_pass<typename C::Fq>(const Affine<typename C::Fq>*, int64_t, uint64_t, const ScalarSort&, Arena&, \
                                                 hipStream_t, MsmBuffers<typename C::Fq>*, EventTimer*);                      \
    template int msm_bucket_pass<typename C::Fq2>(const Affine<typename C::Fq2>*, int64_t, uint64_t, const ScalarSort&,     \
                                                  Arena&, hipStream_t, MsmBuffers<typename C::Fq2>*, EventTimer*);            \
    template int msm_bucket_pass_batch<typename C::Fq>(const PassJob<typename C::Fq>*, int, Arena&, hipStream_t, EventTimer*);   \
    template int msm_bucket_pass_batch<typename C::Fq2>(const PassJob<typename C::Fq2>*, int, Arena&, hipStream_t, EventTimer*); \
    template int msm_reduce<typename C::Fq>(const MsmBuffers<typename C::Fq>&, const ScalarSort&, hipStream_t);             \
    template int msm_reduce_batch<typename C::Fq>(const MsmBuffers<typename C::Fq>* const*, const ScalarSort* const*, int, hipStream_t, bool); \
    template int msm_heavy_reduce<typename C::Fq>(const MsmBuffers<typename C::Fq>&, const ScalarSort&, hipStream_t);     \
    template int msm_heavy_reduce_batch<typename C::Fq>(const MsmBuffers<typename C::Fq>* const*, const ScalarSort* const*, int, hipStream_t); \
    template int msm_reduce<typename C::Fq2>(const MsmBuffers<typename C::Fq2>&, const ScalarSort&, hipStream_t);           \
    template XYZZ<typename C::Fq> fold_windows<typename C::Fq>(const XYZZ<typename C::Fq>*, const MsmPlan&);               \
    template XYZZ<typename C::Fq2> fold_windows<typename C::Fq2>(const XYZZ<typename C::Fq2>*, const MsmPlan&);

// This file is compiled twice (G16_MSM_PART = 0: BLS12-381, 1: BN254) so that the two sets of template instantiations build in parallel.
#ifndef G16_MSM_PART
#define G16_MSM_PART 0
#endif
#if G16_MSM_PART == 0
G16_INSTANTIATE_MSM(Bls12_381)
#else
G16_INSTANTIATE_MSM(Bn254)
#endif

}  // namespace g16
