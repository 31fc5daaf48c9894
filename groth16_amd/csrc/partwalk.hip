// The kernels of the bucket-part walk of the bucket pass (MsmPlan::walk == MSM_WALK_PARTS, part_walk.hpp) and their launchers -- the
// layout (msm_parts_layout) and the pass (msm_parts_pass_launch).  A translation unit and a code object of their own inside the product
// library, so that msm.hip's two objects build as they did without them; the scans are msm.hip's (prefix_scan_u32).
#include "internal.hpp"
#include "fp30.hpp"
#include "acc_store.hpp"
#include "part_walk.hpp"
#include "pass_batch.hpp"

namespace g16 {

// ---------------------------------------------------------------------------------------------
// The bucket-part layout (MSM_WALK_PARTS, part_walk.hpp): slots per bucket = ceil(count / Lmax), and one task descriptor per
//     slot, ordered by length, longest first -- the 64 tasks (32 lane pairs) of a wave then have one trip count, and a launch ends
//     on its shortest tasks.  A counting sort over the <= Lmax lengths (class = Lmax - length):
//   part_count_kernel   a workgroup takes PART_TILE buckets: nparts[], the heavy list, and an LDS histogram of the lengths of their
//                       parts (a bucket's parts have two lengths at most: r = n mod np of q + 1 entries, np - r of q = n / np),
//                       written as one column of the [class][workgroup] count matrix
//   (scans)             nparts -> task_off, and the matrix -> each workgroup's first index in each class
//   part_place_kernel   the same workgroup takes its buckets' index ranges from LDS cursors and writes the descriptors; the
//                       descriptors of a bucket with more than PART_WIDE parts (repeated scalars: one bucket may hold every entry)
//                       are written by the whole workgroup
// No global atomics but the heavy list's; <= 64 registers, Lmax + 3 * PART_WIDE_CAP + 1 words of LDS: they run beside a pass.
// ---------------------------------------------------------------------------------------------
static constexpr uint32_t PART_THREADS = 256, PART_PER_THREAD = PART_TILE / PART_THREADS;   // (PART_TILE, PART_MAX_L: internal.hpp)
static constexpr uint32_t PART_WIDE = 64;         // parts of a bucket one lane still writes alone
static constexpr uint32_t PART_WIDE_CAP = 32;     // wide buckets per workgroup written cooperatively (more: their lanes write them alone)

static __global__ __launch_bounds__(PART_THREADS) void part_count_kernel(const uint32_t* __restrict__ offsets, uint32_t M, uint32_t lmax,
                                                                         uint32_t* __restrict__ nparts, uint32_t* __restrict__ heavy,
                                                                         uint32_t* __restrict__ len_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);   // [lmax]
    for (uint32_t k = threadIdx.x; k < lmax; k += PART_THREADS) hist[k] = 0;
    __syncthreads();
    G16_UNROLL for (uint32_t j = 0; j < PART_PER_THREAD; ++j) {
        const uint32_t b = blockIdx.x * PART_TILE + j * PART_THREADS + threadIdx.x;
        if (b >= M) continue;
        const uint32_t n = offsets[b + 1] - offsets[b];
        const uint32_t np = part_count(n, lmax);
        nparts[b] = np;
        if (np > HEAVY_PARTS) heavy[1 + atomicAdd(&heavy[0], 1u)] = b;
        if (np == 0) continue;
        const uint32_t q = n / np, r = n - q * np;   // 1 <= q <= lmax, and q < lmax when r > 0
        if (r) atomicAdd(&hist[lmax - (q + 1)], r);
        atomicAdd(&hist[lmax - q], np - r);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < lmax; k += PART_THREADS) len_counts[(size_t)k * gridDim.x + blockIdx.x] = hist[k];
}

static __global__ __launch_bounds__(PART_THREADS) void part_place_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ nparts,
                                                                         const uint32_t* __restrict__ task_off, uint32_t M, uint32_t lmax,
                                                                         const uint32_t* __restrict__ len_off, PartTask* __restrict__ tasks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* cur = reinterpret_cast<uint32_t*>(smem);   // [lmax] next index of each length class
    uint32_t* wide = cur + lmax;                           // [1 + 3 * PART_WIDE_CAP] count, then (bucket, first long index, first short index)
    for (uint32_t k = threadIdx.x; k < lmax; k += PART_THREADS) cur[k] = len_off[(size_t)k * gridDim.x + blockIdx.x];
    if (threadIdx.x == 0) wide[0] = 0;
    __syncthreads();
    // part p of a bucket (n = q np + r entries at off, slots from slot0): the long parts take the bucket's range of class q + 1 in
    // order, the short ones its range of class q
    auto put = [&](uint32_t p, uint32_t off, uint32_t q, uint32_t r, uint32_t np, uint32_t slot0, uint32_t at_long, uint32_t at_short) {
        const uint32_t l0 = part_long_before(p, r, np), l1 = part_long_before(p + 1, r, np);
        const bool is_long = l1 != l0;
        const uint32_t idx = is_long ? at_long + l0 : at_short + (p - l0);
        tasks[idx] = PartTask{off + p * q + l0, q + (is_long ? 1u : 0u), slot0 + p};
    };
    G16_UNROLL for (uint32_t j = 0; j < PART_PER_THREAD; ++j) {
        const uint32_t b = blockIdx.x * PART_TILE + j * PART_THREADS + threadIdx.x;
        if (b >= M) continue;
        const uint32_t np = nparts[b];
        if (np == 0) continue;
        const uint32_t off = offsets[b], n = offsets[b + 1] - off;
        const uint32_t q = n / np, r = n - q * np;
        const uint32_t at_long = r ? atomicAdd(&cur[lmax - (q + 1)], r) : 0u;
        const uint32_t at_short = atomicAdd(&cur[lmax - q], np - r);
        if (np > PART_WIDE) {
            const uint32_t w = atomicAdd(&wide[0], 1u);
            if (w < PART_WIDE_CAP) {
                wide[1 + 3 * w] = b; wide[2 + 3 * w] = at_long; wide[3 + 3 * w] = at_short;
                continue;
            }
        }
        const uint32_t slot0 = task_off[b];
        for (uint32_t p = 0; p < np; ++p) put(p, off, q, r, np, slot0, at_long, at_short);
    }
    __syncthreads();
    const uint32_t nwide = min(wide[0], PART_WIDE_CAP);
    for (uint32_t w = 0; w < nwide; ++w) {
        const uint32_t b = wide[1 + 3 * w], np = nparts[b];
        const uint32_t off = offsets[b], n = offsets[b + 1] - off;
        const uint32_t q = n / np, r = n - q * np, slot0 = task_off[b];
        for (uint32_t p = threadIdx.x; p < np; p += PART_THREADS) put(p, off, q, r, np, slot0, wide[2 + 3 * w], wide[3 + 3 * w]);
    }
}

int msm_parts_layout(const uint32_t* counts, uint32_t M, uint32_t lmax, uint32_t* offsets, uint32_t* nparts, uint32_t* task_off, uint32_t* heavy,
                     PartTask* tasks, uint32_t* scratch, hipStream_t st) {
    if (lmax < 8 || lmax > PART_MAX_L || M == 0 || !scratch) return G16_ERR_INTERNAL;
    const uint32_t nblk = (M + PART_TILE - 1) / PART_TILE;
    const uint64_t cells = (uint64_t)lmax * nblk;
    if (cells >= ((uint64_t)1 << 31)) return G16_ERR_INTERNAL;
    uint32_t *len_counts = scratch, *len_off = scratch + cells + 1, *block_sums = scratch + 2 * (cells + 1);   // msm_parts_layout_scratch
    G16_TRY(prefix_scan_u32(counts, offsets, M, 0u, block_sums, st));
    hipLaunchKernelGGL(part_count_kernel, dim3(nblk), dim3(PART_THREADS), (size_t)lmax * sizeof(uint32_t), st, offsets, M, lmax, nparts, heavy,
                       len_counts);
    G16_LAUNCH_CHECK();
    G16_TRY(prefix_scan_u32(nparts, task_off, M, 0u, block_sums, st));
    G16_TRY(prefix_scan_u32(len_counts, len_off, (uint32_t)cells, 0u, block_sums, st));
    hipLaunchKernelGGL(part_place_kernel, dim3(nblk), dim3(PART_THREADS), ((size_t)lmax + 1 + 3 * PART_WIDE_CAP) * sizeof(uint32_t), st, offsets,
                       nparts, task_off, M, lmax, len_off, tasks);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

// the largest v of the wave, in a scalar register
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    G16_UNROLL for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The bucket pass over PARTS (the segment walk: bucket_accumulate30_kernel, msm.hip).  Lane (pair) i of MSM blockIdx.y reads descriptor
// i -- the list is ordered by length, so the wave's tasks have one trip count, or two where it straddles two length classes -- walks
// its entries with the segment walk's software pipeline (walk_bucket_part) and stores its sum once, into its slot.  No search for the
// first bucket, no boundary test, no flush and no slot arithmetic in the loop; the first entry's set and the final store are uniform
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

template <class F30>
int msm_parts_pass_launch(const PassBatch<F30>& batch, const PartTaskBatch& tasks, int n, uint32_t max_tasks, uint32_t M, bool merged,
                          unsigned lds_pad, hipStream_t st) {
    if (n < 1 || n > PASS_BATCH || !max_tasks) return G16_ERR_INTERNAL;
    for (int i = 0; i < n; ++i)
        if (!tasks.tasks[i] || !batch.slot_off[i] || !batch.partials[i]) return G16_ERR_INTERNAL;
    const uint64_t lanes = (uint64_t)max_tasks * F30::LANES_PER_TASK;
    const dim3 grid((unsigned)((lanes + ACC_THREADS - 1) / ACC_THREADS), (unsigned)n);
    hipLaunchKernelGGL((bucket_parts30_kernel<F30>), grid, dim3(ACC_THREADS), lds_pad, st, batch, tasks, M, merged ? 1u : 0u);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

#define PW_INSTANTIATE(F30) \
    template int msm_parts_pass_launch<F30>(const PassBatch<F30>&, const PartTaskBatch&, int, uint32_t, uint32_t, bool, unsigned, hipStream_t);
PW_INSTANTIATE(Fp30<Bls12_381FqP>)
PW_INSTANTIATE(Fp2p30<Bls12_381FqP>)
PW_INSTANTIATE(Fp30<Bn254FqP>)
PW_INSTANTIATE(Fp2p30<Bn254FqP>)

}  // namespace g16
