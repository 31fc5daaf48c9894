// The scalar sort of the MSM (steps 1-4 of msm.hip's map): digit extraction, the counting sorts of the per-window and the merged
// plan, the prefix scans, and the layout tail that turns bucket counts into offsets, partial-sum slots and -- for the bucket-part
// walk (part_walk.hpp) -- the task list.  Nothing here depends on the base field, so the file is built once for both curves; only
// the three kernels that read scalars are templates (on Fr).
#include "internal.hpp"
#include "msm_common.hpp"
#include "part_walk.hpp"
#include <algorithm>
#include <cstdlib>

namespace g16 {

static constexpr int SORT_THREADS = 1024;

struct PlanDev {
    int c, W;
    uint32_t B;
    uint32_t K[10];
    // bucket-space shard (MsmPlan::shard_n): keep the keys with key mod shard_n == shard_r, re-index them as key / shard_n.
    // shard_magic = ceil(2^32 / shard_n): umulhi(key, magic) == key / shard_n exactly for key < 2^20, shard_n <= 64
    // (key * (magic * shard_n - 2^32) < 2^20 * 64 < 2^32).  shard_n == 1: no filter.
    uint32_t shard_n, shard_r, shard_magic;
};

// false: the key belongs to another rank's residue class; true: *key is now the rank's local bucket index
__device__ __forceinline__ bool shard_local_key(const PlanDev& plan, uint32_t* key) {
    if (plan.shard_n <= 1) return true;
    const uint32_t q = __umulhi(*key, plan.shard_magic);
    if (*key - q * plan.shard_n != plan.shard_r) return false;
    *key = q;
    return true;
}

// ---------------------------------------------------------------------------------------------
// 1. digit planes
// ---------------------------------------------------------------------------------------------
// (the body spells out what biased_scalar and window_of below do: written through them it compiles to two or three more instructions
// and two registers fewer, i.e. another kernel, so it stays as measured)
template <class Fr>
__global__ __launch_bounds__(256) void digits_kernel(const Fr* __restrict__ scalars, uint64_t n, PlanDev plan,
                                                     uint16_t* __restrict__ planes) {
    __shared__ uint32_t sw[MSM_SWORDS][256];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t s[Fr::N];
    scalars[i].to_canonical(s);
    uint64_t carry = 0;
    G16_UNROLL for (int k = 0; k < 10; ++k) {
        carry += (uint64_t)(k < Fr::N ? s[k] : 0u) + plan.K[k];
        sw[k][threadIdx.x] = (uint32_t)carry;
        carry >>= 32;
    }
    sw[10][threadIdx.x] = 0;
    // each thread reads back only its own column: no barrier needed
    for (int w = 0; w < plan.W; ++w) {
        const int bit = w * plan.c, word = bit >> 5, sh = bit & 31;
        const uint64_t two = (uint64_t)sw[word][threadIdx.x] | ((uint64_t)sw[word + 1][threadIdx.x] << 32);
        planes[(uint64_t)w * n + i] = (uint16_t)((uint32_t)(two >> sh) & ((1u << plan.c) - 1u));
    }
}

// ---------------------------------------------------------------------------------------------
// 2. histogram   grid = (chunks, W)
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(SORT_THREADS) void bucket_count_kernel(const uint16_t* __restrict__ planes, uint64_t n, uint32_t chunk,
                                                                    int c, uint32_t B, uint32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
    const int w = blockIdx.y;
    for (uint32_t b = threadIdx.x; b < B; b += SORT_THREADS) hist[b] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = min(n, lo + chunk);
    const uint16_t* plane = planes + (uint64_t)w * n;
    for (uint64_t p = lo + threadIdx.x; p < hi; p += SORT_THREADS) {
        uint32_t bucket, neg;
        if (digit_to_bucket(plane[p], c, &bucket, &neg)) atomicAdd(&hist[bucket], 1u);
    }
    __syncthreads();
    uint32_t* out = counts + (uint64_t)w * B;
    for (uint32_t b = threadIdx.x; b < B; b += SORT_THREADS) {
        const uint32_t v = hist[b];
        if (v) atomicAdd(&out[b], v);
    }
}

// ---------------------------------------------------------------------------------------------
// 1m/2m/4m. merged-window variants: every (point, window) digit is an entry of ONE bucket set of 2^(c-1) buckets, cut
// into Q sort classes of 2^blog <= 2^13 buckets (what the LDS histogram holds: SORT_CLASS_LOG below).  Two levels:
//   class_count_kernel / class_partition_kernel   entries -> Q contiguous class regions (block-local LDS cursors on top
//                           of scanned per-(class, block) counts); an entry is a u16 key (bucket in class | sign << 15)
//                           and a u32 tag (point | window << 26)
//   sub_count_kernel / sub_partition_kernel / final_sort_kernel (4m below)   class region -> sub-class regions -> the sorted list,
//                           its last write coalesced.   Sorted entry = point | window << 26 | sign << 31.
//   bucket_count_merged_kernel / bucket_wg_scan_kernel / bucket_scatter_merged_kernel   padded bucket regions only
//                           (G16_MSM_AFFINE_LEVELS > 0): per class an LDS counting sort over the class region, its histograms
//                           exchanged through a [class][workgroup][bucket] matrix instead of global atomics.
// ---------------------------------------------------------------------------------------------
static constexpr int CLASS_THREADS = 256;
static constexpr int MAX_CLASSES = 64;
// The merged counting sort works on SORT CLASSES of 2^13 buckets (round 5; 2^15 before) with 256-lane workgroups: a 32 KB histogram and
// four waves (<= 32 registers each) fit on a compute unit BESIDE eight bucket-pass workgroups (8 x 13 KB of LDS, 2 x 190 / 2 x 239 of a
// SIMD's 512 registers), so h's sort -- which cannot start before the witness map ends, i.e. when the passes begin -- runs underneath the
// passes instead of waiting for a kernel boundary: with 128 KB histograms its count and scatter kernels each sat out a whole 23 ms
// pass and the h pass then waited 2.3 ms for the scatter (kernel trace of round 5).  The sorted list does not depend on the class
// size (classes are contiguous bucket ranges); the reductions keep their own grouping (MsmPlan::B, groups).
static constexpr uint32_t SORT_CLASS_LOG = 13;
static constexpr int SORT_M_THREADS = 256;

// the thread's scalar, biased, as little-endian words in its column of sw
template <class Fr>
__device__ __forceinline__ void biased_scalar(const Fr& sc, const PlanDev& plan, uint32_t (*sw)[CLASS_THREADS]) {
    uint32_t s[Fr::N];
    sc.to_canonical(s);
    uint64_t carry = 0;
    G16_UNROLL for (int k = 0; k < 10; ++k) {
        carry += (uint64_t)(k < Fr::N ? s[k] : 0u) + plan.K[k];
        sw[k][threadIdx.x] = (uint32_t)carry;
        carry >>= 32;
    }
    sw[10][threadIdx.x] = 0;
}
__device__ __forceinline__ uint32_t window_of(const uint32_t (*sw)[CLASS_THREADS], int w, int c) {
    const int bit = w * c, word = bit >> 5, sh = bit & 31;
    const uint64_t two = (uint64_t)sw[word][threadIdx.x] | ((uint64_t)sw[word + 1][threadIdx.x] << 32);
    return (uint32_t)(two >> sh) & ((1u << c) - 1u);
}

// block_counts[q * gridDim.x + block] = entries of class q among this block's 256 points
template <class Fr>
__global__ __launch_bounds__(CLASS_THREADS) void class_count_kernel(const Fr* __restrict__ scalars, uint64_t n, PlanDev plan, uint32_t blog,
                                                                    uint32_t Q, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t sw[MSM_SWORDS][CLASS_THREADS];
    __shared__ uint32_t cnt[MAX_CLASSES];
    if (threadIdx.x < MAX_CLASSES) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * CLASS_THREADS + threadIdx.x;
    if (i < n) {
        biased_scalar(scalars[i], plan, sw);
        for (int w = 0; w < plan.W; ++w) {
            uint32_t key, neg;
            if (digit_to_bucket(window_of(sw, w, plan.c), plan.c, &key, &neg) && shard_local_key(plan, &key)) atomicAdd(&cnt[key >> blog], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < Q) block_counts[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

template <class Fr>
__global__ __launch_bounds__(CLASS_THREADS) void class_partition_kernel(const Fr* __restrict__ scalars, uint64_t n, PlanDev plan, uint32_t blog,
                                                                        uint32_t Q, const uint32_t* __restrict__ block_off,
                                                                        uint16_t* __restrict__ ent_key, uint32_t* __restrict__ ent_tag) {
    __shared__ uint32_t sw[MSM_SWORDS][CLASS_THREADS];
    __shared__ uint32_t cur[MAX_CLASSES];
    if (threadIdx.x < Q) cur[threadIdx.x] = block_off[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * CLASS_THREADS + threadIdx.x;
    if (i >= n) return;
    biased_scalar(scalars[i], plan, sw);
    for (int w = 0; w < plan.W; ++w) {
        uint32_t key, neg;
        if (digit_to_bucket(window_of(sw, w, plan.c), plan.c, &key, &neg) && shard_local_key(plan, &key)) {
            const uint32_t pos = atomicAdd(&cur[key >> blog], 1u);
            ent_key[pos] = (uint16_t)((key & ((1u << blog) - 1u)) | (neg << 15));
            ent_tag[pos] = (uint32_t)i | ((uint32_t)w << 26);
        }
    }
}

// grid = (G, Q): workgroup (x, q) owns the tiles x, x + G, x + 2G, ... (SORT_M_THREADS entries each) of class region q.
// NO global atomics (round 5).  The first version flushed every workgroup's histogram with one global atomic per non-empty bucket and
// reserved scatter slices with one RETURNING global atomic per non-empty bucket: 2048 workgroups x ~18 000 buckets = 37 M device-scope
// atomics per kernel at 2^22 -- on this GPU those are performed at the memory side (eight XCDs, eight L2s) -- 0.9 ms for the count and
// 2.5 ms for the scatter of a 54.5 M-entry sort whose compulsory traffic is ~1.3 GB.  Now each workgroup STORES its histogram as one
// row of a [class][workgroup][bucket] matrix (coalesced), a small kernel turns the columns into exclusive prefixes over the
// workgroups (one thread per bucket, coalesced across threads) and totals, and the scatter reads its row back: its slice of bucket b
// starts at offsets[b] + prefix[workgroup][b].  The scatter no longer re-counts its tiles either.
static __global__ __launch_bounds__(SORT_M_THREADS) void bucket_count_merged_kernel(const uint16_t* __restrict__ ent_key,
                                                                           const uint32_t* __restrict__ class_off, uint32_t nb, uint32_t B,
                                                                           uint32_t* __restrict__ wg_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
    const uint32_t q = blockIdx.y;
    const uint32_t lo = class_off[(uint64_t)q * nb], hi = class_off[(uint64_t)(q + 1) * nb];
    for (uint32_t b = threadIdx.x; b < B; b += SORT_M_THREADS) hist[b] = 0;
    __syncthreads();
    for (uint64_t p = (uint64_t)lo + blockIdx.x * SORT_M_THREADS + threadIdx.x; p < hi; p += (uint64_t)gridDim.x * SORT_M_THREADS)
        atomicAdd(&hist[ent_key[p] & 0x7fffu], 1u);
    __syncthreads();
    uint32_t* out = wg_counts + ((uint64_t)q * gridDim.x + blockIdx.x) * B;   // a workgroup without tiles stores its row of zeros
    for (uint32_t b = threadIdx.x; b < B; b += SORT_M_THREADS) out[b] = hist[b];
}

// one thread per (class, bucket): wg_counts[q][x][b] <- sum of the rows x' < x (in place), counts[q * B + b] <- the column's total
static __global__ __launch_bounds__(256) void bucket_wg_scan_kernel(uint32_t* __restrict__ wg_counts, uint32_t G, uint32_t B, uint32_t M,
                                                                    uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const uint32_t q = i / B, b = i - q * B;
    uint32_t* col = wg_counts + (uint64_t)q * G * B + b;
    uint32_t run = 0;
    for (uint32_t x = 0; x < G; ++x) {
        const uint32_t v = col[(uint64_t)x * B];
        col[(uint64_t)x * B] = run;
        run += v;
    }
    counts[i] = run;
}

static __global__ __launch_bounds__(SORT_M_THREADS) void bucket_scatter_merged_kernel(const uint16_t* __restrict__ ent_key,
                                                                             const uint32_t* __restrict__ ent_tag,
                                                                             const uint32_t* __restrict__ class_off, uint32_t nb, uint32_t B,
                                                                             const uint32_t* __restrict__ offsets,
                                                                             const uint32_t* __restrict__ wg_counts, uint32_t* __restrict__ sorted) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
    const uint32_t q = blockIdx.y;
    const uint32_t lo = class_off[(uint64_t)q * nb], hi = class_off[(uint64_t)(q + 1) * nb];
    if ((uint64_t)lo + (uint64_t)blockIdx.x * SORT_M_THREADS >= hi) return;
    // hist[b] = this workgroup's write cursor in bucket b: the bucket's offset + what the workgroups before this one put there
    const uint64_t qb = (uint64_t)q * B;
    const uint32_t* mine = wg_counts + ((uint64_t)q * gridDim.x + blockIdx.x) * B;
    for (uint32_t b = threadIdx.x; b < B; b += SORT_M_THREADS) hist[b] = offsets[qb + b] + mine[b];
    __syncthreads();
    const uint64_t first = (uint64_t)lo + blockIdx.x * SORT_M_THREADS + threadIdx.x, step = (uint64_t)gridDim.x * SORT_M_THREADS;
    for (uint64_t p = first; p < hi; p += step) {
        const uint32_t d = ent_key[p];
        const uint32_t pos = atomicAdd(&hist[d & 0x7fffu], 1u);
        sorted[pos] = ent_tag[p] | ((d >> 15) << 31);
    }
}

// ---------------------------------------------------------------------------------------------
// 3. scans over the M = W*B buckets: an exclusive prefix sum of a u32 array in three small coalesced launches
//    (block sums -> scan of block sums -> write), 2048 values per workgroup.  Used for bucket counts -> bucket offsets,
//    per-bucket partial-slot counts -> slot offsets, and the part layout's length matrix (prefix_scan_u32, the one launcher).
// ---------------------------------------------------------------------------------------------
static constexpr int SCAN_THREADS = 256;
static constexpr int SCAN_PER_THREAD = 8;
static constexpr int SCAN_TILE = SCAN_THREADS * SCAN_PER_THREAD;

// exclusive scan of one value per thread across the workgroup; returns the workgroup total through *total
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* sh, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_THREADS; d <<= 1) {
        const uint32_t add = tid >= d ? sh[tid - d] : 0u;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = sh[tid];
    *total = sh[SCAN_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// `pad` (a power of two minus one, or 0): every value is rounded up to a multiple of pad + 1 before it is summed -- bucket
// regions of the batched-affine plan start and end on multiples of 2^R entries
static __global__ __launch_bounds__(SCAN_THREADS) void scan_block_sums_kernel(const uint32_t* __restrict__ vals, uint32_t M, uint32_t pad,
                                                                       uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t sa[SCAN_THREADS];
    const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD;
    uint32_t sum = 0, tot;
    G16_UNROLL for (int j = 0; j < SCAN_PER_THREAD; ++j) sum += (base + j < M) ? ((vals[base + j] + pad) & ~pad) : 0u;
    (void)block_exclusive(sum, sa, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

static __global__ __launch_bounds__(SCAN_THREADS) void scan_block_offsets_kernel(uint32_t* __restrict__ block_sums, uint32_t nblocks, uint32_t M,
                                                                          uint32_t* __restrict__ prefix) {
    __shared__ uint32_t sa[SCAN_THREADS];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t a = i < nblocks ? block_sums[i] : 0u;
        uint32_t tot;
        const uint32_t ea = block_exclusive(a, sa, &tot);
        if (i < nblocks) block_sums[i] = carry + ea;
        carry += tot;
    }
    if (threadIdx.x == 0) prefix[M] = carry;
}

static __global__ __launch_bounds__(SCAN_THREADS) void scan_write_kernel(const uint32_t* __restrict__ vals, uint32_t M, uint32_t pad,
                                                                  const uint32_t* __restrict__ block_base, uint32_t* __restrict__ prefix) {
    __shared__ uint32_t sa[SCAN_THREADS];
    const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD;
    uint32_t cv[SCAN_PER_THREAD], sum = 0, tot;
    G16_UNROLL for (int j = 0; j < SCAN_PER_THREAD; ++j) { cv[j] = (base + j < M) ? ((vals[base + j] + pad) & ~pad) : 0u; sum += cv[j]; }
    uint32_t a = block_base[blockIdx.x] + block_exclusive(sum, sa, &tot);
    G16_UNROLL for (int j = 0; j < SCAN_PER_THREAD; ++j) {
        if (base + j < M) { prefix[base + j] = a; a += cv[j]; }
    }
}

// partial-sum slots of bucket b = number of length-L segments of the sorted list its entries touch
// (batched-affine plan: the bucket pass walks the level-R list, whose bucket regions are offsets >> R)
static __global__ void bucket_slots_kernel(const uint32_t* __restrict__ offsets, uint32_t M, uint32_t off_shift, uint32_t lseg,
                                    uint32_t* __restrict__ nparts, uint32_t* __restrict__ heavy /* [0] = count, then bucket ids */) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= M) return;
    const uint32_t lo = offsets[b] >> off_shift, hi = offsets[b + 1] >> off_shift;
    const uint32_t np = hi > lo ? ((hi - 1) / lseg - lo / lseg + 1u) : 0u;
    nparts[b] = np;
    if (np > HEAVY_PARTS) heavy[1 + atomicAdd(&heavy[0], 1u)] = b;
}

// ---------------------------------------------------------------------------------------------
// 4m. merged plan without padded bucket regions (affine_levels == 0): second partition level + LDS-resident final level.
// The scatter above puts every word at a random position of a 3.4 MB class region -- a memory sector dirtied for 4 useful bytes,
// 1.2 ms for 54.5 M entries, and the partial-line traffic slows the witness map's first sweep beside it.  Instead:
//   sub_count_kernel / sub_partition_kernel   class region -> S sub-class regions of 2^sublog consecutive buckets (2^6 at 2^22, c = 20:
//                           ~6.7 K entries each).  A workgroup stages a tile of SUB_TILE entries in LDS, ordered by sub-class, and
//                           streams it out: every destination gets a run of consecutive words from consecutive lanes.  Cursors come
//                           from a [class][sub-class][workgroup] count matrix and one prefix scan, as on the class level.
//   final_sort_kernel       one workgroup per sub-class: LDS histogram of its <= 128 buckets -> counts[], scan, entries placed by
//                           bucket in LDS, the slice of `sorted` streamed out coalesced.  With unpadded regions a bucket's offset is
//                           the sub-class region's start + the scanned histogram, so this level needs neither `offsets` nor a count
//                           pass of its own.  A sub-class with more than FINAL_CAP entries (repeated scalars; the top window's short
//                           digit range doubles the load of the first 2^15 buckets) is detected from its region's bounds and scattered
//                           directly through the same LDS cursors: 2^sublog open runs per workgroup instead of 2^13.
// No global atomics.  <= 64 registers, <= 48 KB of LDS per 256-lane workgroup: the kernels run beside the G2 bucket pass like the
// ones they replace (tests/test_sort_kernel_resources.py).
// ---------------------------------------------------------------------------------------------
static constexpr uint32_t MAX_SUBS = 256;        // sub-classes per class
static constexpr uint32_t MAX_SUB_LOG = 7;       // buckets per sub-class <= 128
static constexpr uint32_t SUB_TILE = 4096;       // entries staged per step of the sub-class partition: runs of ~32 per destination
static constexpr uint32_t SUB_PER_LANE = SUB_TILE / SORT_M_THREADS;
static constexpr uint32_t SUB_BATCH = 4;         // loads in flight per lane in the partition's loops
static constexpr uint32_t FINAL_CAP = 10240;     // entries of a sub-class the final level holds in LDS (40 KB of sorted words)
static constexpr uint32_t FINAL_BATCH = 4;       // loads in flight per lane in the final level's loops
static_assert(SORT_M_THREADS == SCAN_THREADS && MAX_SUBS <= SCAN_THREADS && SUB_TILE <= 65536, "block_exclusive scans one value per lane");

// One step of an LDS counter per valid lane, returning the value before the step.  A wave whose valid lanes all hit ONE counter
// (a repeated scalar: every entry of the region in one bucket) takes its slots with a single atomic instead of 64 serialised ones.
// Every lane of the wave must call it.
__device__ __forceinline__ uint32_t lds_take(uint32_t* ctr, uint32_t idx, bool valid) {
    const uint64_t act = __ballot(valid);
    if (act == 0) return 0;
    const int first = __ffsll((unsigned long long)act) - 1;
    const uint32_t idx0 = (uint32_t)__shfl((int)idx, first);
    if (__ballot(valid && idx == idx0) == act) {
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t base = 0;
        if ((int)lane == first) base = atomicAdd(&ctr[idx0], (uint32_t)__popcll(act));
        base = (uint32_t)__shfl((int)base, first);
        return base + (uint32_t)__popcll(act & (((uint64_t)1 << lane) - 1u));
    }
    return valid ? atomicAdd(&ctr[idx], 1u) : 0u;
}

// grid = (G, Q): workgroup (x, q) owns the tiles x, x + G, ... (SUB_TILE entries each) of class region q.
// sub_counts[(q * S + s) * G + x] = its entries of sub-class s -- the order in which the exclusive scan of the matrix yields its cursors
static __global__ __launch_bounds__(SORT_M_THREADS) void sub_count_kernel(const uint16_t* __restrict__ ent_key,
                                                                          const uint32_t* __restrict__ class_off, uint32_t nb, uint32_t S,
                                                                          uint32_t sublog, uint32_t* __restrict__ sub_counts) {
    __shared__ uint32_t cnt[MAX_SUBS];
    const uint32_t q = blockIdx.y;
    const uint64_t lo = class_off[(uint64_t)q * nb], hi = class_off[(uint64_t)(q + 1) * nb];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t tlo = lo + (uint64_t)blockIdx.x * SUB_TILE; tlo < hi; tlo += (uint64_t)gridDim.x * SUB_TILE) {
        uint32_t k[SUB_PER_LANE];
        G16_UNROLL for (uint32_t j = 0; j < SUB_PER_LANE; ++j) {
            const uint64_t p = tlo + j * SORT_M_THREADS + threadIdx.x;
            k[j] = p < hi ? (uint32_t)ent_key[p] : 0xffffffffu;
        }
        G16_UNROLL for (uint32_t j = 0; j < SUB_PER_LANE; ++j) (void)lds_take(cnt, (k[j] & 0x7fffu) >> sublog, k[j] != 0xffffffffu);
    }
    __syncthreads();
    if (threadIdx.x < S) sub_counts[((uint64_t)q * S + threadIdx.x) * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

static __global__ __launch_bounds__(SORT_M_THREADS) void sub_partition_kernel(const uint16_t* __restrict__ ent_key,
                                                                              const uint32_t* __restrict__ ent_tag,
                                                                              const uint32_t* __restrict__ class_off, uint32_t nb, uint32_t S,
                                                                              uint32_t sublog, const uint32_t* __restrict__ sub_off,
                                                                              uint16_t* __restrict__ out_key, uint32_t* __restrict__ out_tag) {
    __shared__ uint32_t cnt[MAX_SUBS], start[MAX_SUBS], cur[MAX_SUBS], gcur[MAX_SUBS], sa[SCAN_THREADS];
    __shared__ uint32_t stag[SUB_TILE];
    __shared__ uint16_t skey[SUB_TILE];
    const uint32_t q = blockIdx.y;
    const uint64_t lo = class_off[(uint64_t)q * nb], hi = class_off[(uint64_t)(q + 1) * nb];
    if (lo + (uint64_t)blockIdx.x * SUB_TILE >= hi) return;
    gcur[threadIdx.x] = threadIdx.x < S ? sub_off[((uint64_t)q * S + threadIdx.x) * gridDim.x + blockIdx.x] : 0u;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t tlo = lo + (uint64_t)blockIdx.x * SUB_TILE; tlo < hi; tlo += (uint64_t)gridDim.x * SUB_TILE) {
        const uint32_t tn = (uint32_t)min((uint64_t)SUB_TILE, hi - tlo);
        // two rolled loops, SUB_BATCH loads in flight per lane: count the tile, scan, then take the staging slots from the scanned
        // cursors (the keys come from the cache the second time; ranks kept in registers would cost sixteen of them)
        _Pragma("unroll 1") for (uint32_t i0 = 0; i0 < tn; i0 += SUB_BATCH * SORT_M_THREADS) {
            uint32_t k[SUB_BATCH];
            G16_UNROLL for (uint32_t j = 0; j < SUB_BATCH; ++j) {
                const uint32_t i = i0 + j * SORT_M_THREADS + threadIdx.x;
                k[j] = i < tn ? (uint32_t)ent_key[tlo + i] : 0xffffffffu;
            }
            G16_UNROLL for (uint32_t j = 0; j < SUB_BATCH; ++j) (void)lds_take(cnt, (k[j] & 0x7fffu) >> sublog, k[j] != 0xffffffffu);
        }
        __syncthreads();
        uint32_t tot;
        const uint32_t mine = cnt[threadIdx.x], ex = block_exclusive(mine, sa, &tot);
        start[threadIdx.x] = ex;
        cur[threadIdx.x] = ex;
        __syncthreads();
        _Pragma("unroll 1") for (uint32_t i0 = 0; i0 < tn; i0 += SUB_BATCH * SORT_M_THREADS) {
            uint32_t k[SUB_BATCH], t[SUB_BATCH];
            G16_UNROLL for (uint32_t j = 0; j < SUB_BATCH; ++j) {
                const uint32_t i = i0 + j * SORT_M_THREADS + threadIdx.x;
                k[j] = i < tn ? (uint32_t)ent_key[tlo + i] : 0xffffffffu;
                t[j] = i < tn ? ent_tag[tlo + i] : 0u;
            }
            G16_UNROLL for (uint32_t j = 0; j < SUB_BATCH; ++j) {
                const bool valid = k[j] != 0xffffffffu;
                const uint32_t pos = lds_take(cur, (k[j] & 0x7fffu) >> sublog, valid);
                if (valid) {
                    skey[pos] = (uint16_t)k[j];
                    stag[pos] = t[j];
                }
            }
        }
        __syncthreads();
        // staged position i belongs to sub-class s at rank i - start[s]: consecutive lanes, consecutive words of s's region
        _Pragma("unroll 1") for (uint32_t i = threadIdx.x; i < tn; i += SORT_M_THREADS) {
            const uint32_t key = skey[i], s = (key & 0x7fffu) >> sublog;
            const uint32_t g = gcur[s] + (i - start[s]);
            out_key[g] = (uint16_t)key;
            out_tag[g] = stag[i];
        }
        __syncthreads();
        gcur[threadIdx.x] += mine;
        cnt[threadIdx.x] = 0;
        __syncthreads();
    }
}

// grid = Q * S: workgroup u owns sub-class u = buckets [u << sublog, (u + 1) << sublog), entries [sub_off[u * G], sub_off[(u + 1) * G])
static __global__ __launch_bounds__(SORT_M_THREADS) void final_sort_kernel(const uint16_t* __restrict__ ent_key,
                                                                           const uint32_t* __restrict__ ent_tag,
                                                                           const uint32_t* __restrict__ sub_off, uint32_t G, uint32_t sublog,
                                                                           uint32_t* __restrict__ counts, uint32_t* __restrict__ sorted) {
    __shared__ uint32_t cnt[1u << MAX_SUB_LOG], cur[1u << MAX_SUB_LOG], sa[SCAN_THREADS];
    __shared__ uint32_t out[FINAL_CAP];
    const uint32_t u = blockIdx.x, NB = 1u << sublog;
    const uint64_t lo = sub_off[(uint64_t)u * G], hi = sub_off[(uint64_t)(u + 1) * G];
    if (threadIdx.x < NB) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t base = lo; base < hi; base += 2 * FINAL_BATCH * SORT_M_THREADS) {
        uint32_t k[2 * FINAL_BATCH];
        G16_UNROLL for (uint32_t j = 0; j < 2 * FINAL_BATCH; ++j) {
            const uint64_t p = base + j * SORT_M_THREADS + threadIdx.x;
            k[j] = p < hi ? (uint32_t)ent_key[p] : 0xffffffffu;
        }
        G16_UNROLL for (uint32_t j = 0; j < 2 * FINAL_BATCH; ++j) (void)lds_take(cnt, k[j] & (NB - 1u), k[j] != 0xffffffffu);
    }
    __syncthreads();
    const uint32_t mine = threadIdx.x < NB ? cnt[threadIdx.x] : 0u;
    if (threadIdx.x < NB) counts[((uint64_t)u << sublog) + threadIdx.x] = mine;
    uint32_t tot;
    const uint32_t ex = block_exclusive(mine, sa, &tot);
    if (threadIdx.x < NB) cur[threadIdx.x] = ex;
    __syncthreads();
    const bool resident = hi - lo <= FINAL_CAP;   // workgroup-uniform
    for (uint64_t base = lo; base < hi; base += FINAL_BATCH * SORT_M_THREADS) {
        uint32_t k[FINAL_BATCH], t[FINAL_BATCH];
        G16_UNROLL for (uint32_t j = 0; j < FINAL_BATCH; ++j) {
            const uint64_t p = base + j * SORT_M_THREADS + threadIdx.x;
            k[j] = p < hi ? (uint32_t)ent_key[p] : 0xffffffffu;
            t[j] = p < hi ? ent_tag[p] : 0u;
        }
        G16_UNROLL for (uint32_t j = 0; j < FINAL_BATCH; ++j) {
            const bool valid = k[j] != 0xffffffffu;
            const uint32_t pos = lds_take(cur, k[j] & (NB - 1u), valid), word = t[j] | ((k[j] >> 15) << 31);
            if (valid) {
                if (resident) out[pos] = word;
                else sorted[lo + pos] = word;
            }
        }
    }
    if (!resident) return;
    __syncthreads();
    const uint32_t N = (uint32_t)(hi - lo);
    for (uint32_t i = threadIdx.x; i < N; i += SORT_M_THREADS) sorted[lo + i] = out[i];
}

// ---------------------------------------------------------------------------------------------
// 4. scatter   grid = (chunks, W)
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(SORT_THREADS) void bucket_scatter_kernel(const uint16_t* __restrict__ planes, uint64_t n, uint32_t chunk,
                                                                      int c, uint32_t B, const uint32_t* __restrict__ offsets,
                                                                      uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
    const int w = blockIdx.y;
    for (uint32_t b = threadIdx.x; b < B; b += SORT_THREADS) hist[b] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * chunk, hi = min(n, lo + chunk);
    const uint16_t* plane = planes + (uint64_t)w * n;
    for (uint64_t p = lo + threadIdx.x; p < hi; p += SORT_THREADS) {
        uint32_t bucket, neg;
        if (digit_to_bucket(plane[p], c, &bucket, &neg)) atomicAdd(&hist[bucket], 1u);
    }
    __syncthreads();
    // reserve a slice of every non-empty bucket; hist[b] becomes this block's write cursor
    const uint64_t wb = (uint64_t)w * B;
    for (uint32_t b = threadIdx.x; b < B; b += SORT_THREADS) {
        const uint32_t v = hist[b];
        if (v) hist[b] = offsets[wb + b] + atomicAdd(&cursor[wb + b], v);
    }
    __syncthreads();
    for (uint64_t p = lo + threadIdx.x; p < hi; p += SORT_THREADS) {
        uint32_t bucket, neg;
        if (digit_to_bucket(plane[p], c, &bucket, &neg)) {
            const uint32_t pos = atomicAdd(&hist[bucket], 1u);
            sorted[pos] = (uint32_t)p | (neg << 31);
        }
    }
}

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

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// exclusive prefix sum of `count` values (3. above; internal.hpp); block_sums: scratch of ceil(count / SCAN_TILE) words
int prefix_scan_u32(const uint32_t* vals, uint32_t* prefix, uint32_t count, uint32_t padmask, uint32_t* block_sums, hipStream_t st) {
    const uint32_t nblocks = (count + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(nblocks), dim3(SCAN_THREADS), 0, st, vals, count, padmask, block_sums);
    G16_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_block_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, block_sums, nblocks, count, prefix);
    G16_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_write_kernel, dim3(nblocks), dim3(SCAN_THREADS), 0, st, vals, count, padmask, block_sums, prefix);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

// The layout tail of a sort for the segment walk, which the pass lab (unit_api.hpp) runs on caller-made counts: bucket counts ->
// offsets (every count rounded up to a multiple of 2^R), offsets -> partial-sum slots per bucket and the heavy list, slots -> task_off.
int msm_slot_layout(const uint32_t* counts, uint32_t M, int R, uint32_t lseg, uint32_t* offsets, uint32_t* nparts, uint32_t* task_off,
                    uint32_t* heavy, uint32_t* block_sums, hipStream_t st) {
    G16_TRY(prefix_scan_u32(counts, offsets, M, (1u << R) - 1u, block_sums, st));
    hipLaunchKernelGGL(bucket_slots_kernel, dim3((M + 255) / 256), dim3(256), 0, st, offsets, M, (uint32_t)R, lseg, nparts, heavy);
    G16_LAUNCH_CHECK();
    G16_TRY(prefix_scan_u32(nparts, task_off, M, 0u, block_sums, st));
    return G16_OK;
}

// the same tail for the bucket-part walk (the layout above)
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

// The four kernels whose LDS histogram is dynamic may take 128 KiB of it (2^15 buckets); every host path that launches one of them
// comes through here first.
static int raise_histogram_lds_limit() {
    static PerDeviceOnce attr_once;
    std::atomic<bool>& attr_set = attr_once.flag();
    if (attr_set) return G16_OK;
    for (const void* kernel : {reinterpret_cast<const void*>(&bucket_count_kernel), reinterpret_cast<const void*>(&bucket_scatter_kernel),
                               reinterpret_cast<const void*>(&bucket_count_merged_kernel),
                               reinterpret_cast<const void*>(&bucket_scatter_merged_kernel)})
        G16_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    attr_set = true;
    return G16_OK;
}

// The per-window sort from its second step on, over W planes of n u16 digits (out->plan and out->n are set): histogram, slot layout,
// scatter.  R: the padding level of the batched-affine plan -- every bucket region is padded to a multiple of 2^R entries; the padding
// slots keep the hole word the list is pre-filled with, and the bucket pass walks the level-R list (1 / 2^R of the slots).
static int sort_planes(const uint16_t* planes, int R, Arena& arena, hipStream_t st, ScalarSort* out) {
    const MsmPlan& plan = out->plan;
    const uint64_t n = out->n;
    const uint32_t M = plan.buckets();
    const uint64_t max_sorted = n * (uint64_t)plan.W + (uint64_t)M * ((1u << R) - 1u);
    if (max_sorted >= ((uint64_t)1 << 32)) return G16_ERR_BAD_LENGTH;
    uint32_t *counts = nullptr, *nparts = nullptr, *block_sums = nullptr;
    G16_TRY(arena.alloc_n((size_t)3 * M + 1, &counts));  // counts | scatter cursors | heavy count + list
    uint32_t* cursor = counts + M;
    out->heavy = counts + 2 * (size_t)M;
    G16_TRY(arena.alloc_n((size_t)M + 1, &out->offsets));
    G16_TRY(arena.alloc_n((size_t)M + 1, &out->task_off));
    G16_TRY(arena.alloc_n((size_t)M, &nparts));
    G16_TRY(arena.alloc_n((size_t)(M + SCAN_TILE - 1) / SCAN_TILE, &block_sums));
    out->max_sorted = max_sorted;
    G16_TRY(arena.alloc_n(max_sorted ? max_sorted : 1, &out->sorted));
    if (R) G16_HIP_TRY(hipMemsetAsync(out->sorted, 0xff, max_sorted * sizeof(uint32_t), st));   // SORT_HOLE
    out->max_segments = (uint32_t)(((max_sorted >> R) + plan.Lmax - 1) / plan.Lmax);
    out->max_tasks = out->max_segments + M;   // a bucket gets one slot per segment it touches: <= segments + buckets in total
    G16_HIP_TRY(hipMemsetAsync(counts, 0, ((size_t)2 * M + 1) * sizeof(uint32_t), st));
    const size_t lds = (size_t)plan.B * sizeof(uint32_t);
    G16_TRY(raise_histogram_lds_limit());
    const unsigned nchunks = (unsigned)((n + plan.chunk - 1) / plan.chunk);
    if (n) {
        hipLaunchKernelGGL(bucket_count_kernel, dim3(nchunks, plan.W), dim3(SORT_THREADS), lds, st, planes, n, plan.chunk, plan.c, plan.B,
                           counts);
        G16_LAUNCH_CHECK();
    }
    G16_TRY(msm_slot_layout(counts, M, R, plan.Lmax, out->offsets, nparts, out->task_off, out->heavy, block_sums, st));
    if (n) {
        hipLaunchKernelGGL(bucket_scatter_kernel, dim3(nchunks, plan.W), dim3(SORT_THREADS), lds, st, planes, n, plan.chunk, plan.c, plan.B,
                           out->offsets, cursor, out->sorted);
        G16_LAUNCH_CHECK();
    }
    return G16_OK;
}

// Short scalars (the ceremony library's 128-bit coefficients, coeffs128_plan): the per-window path over digit planes the caller made
// with a kernel of its own (W planes of n u16 digits of scalar + K, as digits_kernel writes them) -- unchanged kernels.
int sort_digit_planes(const MsmPlan& plan, const uint16_t* planes, uint64_t n, Arena& arena, hipStream_t st, ScalarSort* out) {
    if (plan.merged || plan.affine_levels || n >= ((uint64_t)1 << 31)) return G16_ERR_INTERNAL;
    out->plan = plan;
    out->n = n;
    return sort_planes(planes, 0, arena, st, out);
}

static int ilog2(uint32_t v) { int l = 0; while ((1u << l) < v) ++l; return l; }

template <class C>
int sort_scalars(const typename C::Fr* d_scalars, uint64_t n, int merged_c, Arena& arena, hipStream_t st, ScalarSort* out, int shard_n,
                 int shard_r, int walk) {
    typedef typename C::Fr Fr;
    if (n >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
    uint32_t modw[Fr::N];
    for (int i = 0; i < Fr::N; ++i) modw[i] = Fr::Params::mod(i);
    MsmPlan plan;
    G16_TRY(make_msm_plan(n, Fr::Params::BITS, modw, Fr::N, merged_c, &plan, shard_n, shard_r));
    // the bucket-part walk: merged plans whose pass walks the sorted list itself (and lengths its layout's histogram holds)
    const bool parts = walk == MSM_WALK_PARTS && plan.merged && plan.affine_levels == 0 && plan.Lmax <= PART_MAX_L;
    plan.walk = parts ? MSM_WALK_PARTS : MSM_WALK_SEGMENT;
    out->plan = plan;
    out->n = n;
    const uint32_t M = plan.buckets();
    const uint64_t nw = n * (uint64_t)plan.W;
    if (nw >= ((uint64_t)1 << 32)) return G16_ERR_BAD_LENGTH;
    PlanDev pd;
    pd.c = plan.c; pd.W = plan.W; pd.B = plan.B;
    for (int k = 0; k < 10; ++k) pd.K[k] = plan.K[k];
    pd.shard_n = (uint32_t)plan.shard_n;
    pd.shard_r = (uint32_t)plan.shard_r;
    pd.shard_magic = plan.shard_n > 1 ? (uint32_t)((((uint64_t)1 << 32) + (uint64_t)plan.shard_n - 1) / (uint64_t)plan.shard_n) : 0u;
    const int R = plan.affine_levels;
    uint16_t* planes = nullptr;     // per-window plan: digit planes; merged plan: entry keys, class-partitioned
    G16_TRY(arena.alloc_n(nw ? nw : 1, &planes));
    if (!plan.merged) {
        if (n) {
            hipLaunchKernelGGL((digits_kernel<Fr>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_scalars, n, pd, planes);
            G16_LAUNCH_CHECK();
        }
        return sort_planes(planes, R, arena, st, out);
    }
    uint32_t* ent_tag = nullptr;    // entry tags (point | window << 26), class-partitioned
    uint32_t *class_cnt = nullptr, *class_off = nullptr;
    uint32_t *counts = nullptr, *nparts = nullptr, *block_sums = nullptr;
    // sort classes of Bs = 2^13 buckets (or the whole bucket set when it is smaller)
    uint32_t sort_class_log = SORT_CLASS_LOG;
    if (const char* e = getenv("G16_SORT_CLASS_LOG")) {   // A/B: 15 = histograms of 128 KB (no room beside the bucket passes)
        const int v = atoi(e);
        if (v >= 8 && v <= 15) sort_class_log = (uint32_t)v;
    }
    const uint32_t slog = std::min<uint32_t>(sort_class_log, (uint32_t)ilog2(plan.B));
    const uint32_t Bs = 1u << slog;
    const uint32_t nb = (uint32_t)((n + CLASS_THREADS - 1) / CLASS_THREADS), Q = M >> slog;
    if (Q > MAX_CLASSES) return G16_ERR_INTERNAL;
    G16_TRY(arena.alloc_n(nw ? nw : 1, &ent_tag));
    G16_TRY(arena.alloc_n((size_t)Q * nb + 1, &class_cnt));
    G16_TRY(arena.alloc_n((size_t)Q * nb + 1, &class_off));
    G16_TRY(arena.alloc_n((size_t)3 * M + 1, &counts));  // counts | (the per-window scatter's cursors) | heavy count + list
    out->heavy = counts + 2 * (size_t)M;
    G16_TRY(arena.alloc_n((size_t)M + 1, &out->offsets));
    G16_TRY(arena.alloc_n((size_t)M + 1, &out->task_off));
    G16_TRY(arena.alloc_n((size_t)M, &nparts));
    const uint64_t max_sorted = nw + (uint64_t)M * ((1u << R) - 1u);   // padded bucket regions (the batched-affine plan, sort_planes above)
    if (max_sorted >= ((uint64_t)1 << 32)) return G16_ERR_BAD_LENGTH;
    out->max_sorted = max_sorted;
    G16_TRY(arena.alloc_n(max_sorted ? max_sorted : 1, &out->sorted));
    if (R) G16_HIP_TRY(hipMemsetAsync(out->sorted, 0xff, max_sorted * sizeof(uint32_t), st));   // SORT_HOLE
    out->max_segments = (uint32_t)(((max_sorted >> R) + plan.Lmax - 1) / plan.Lmax);
    out->max_tasks = out->max_segments + M;   // a bucket gets one slot per segment it touches: <= segments + buckets in total
    uint32_t* part_scratch = nullptr;
    if (parts) {
        // sum_b ceil(n_b / Lmax) <= entries / Lmax + buckets; one task per slot, and the grid of the pass covers that bound
        out->max_tasks = (uint32_t)(nw / plan.Lmax) + M;
        out->max_segments = out->max_tasks;
        G16_TRY(arena.alloc_n((size_t)out->max_tasks ? out->max_tasks : 1, &out->tasks));
        G16_TRY(arena.alloc_n(msm_parts_layout_scratch(M, plan.Lmax), &part_scratch));
    }
    G16_HIP_TRY(hipMemsetAsync(counts, 0, ((size_t)2 * M + 1) * sizeof(uint32_t), st));
    const size_t lds = (size_t)Bs * sizeof(uint32_t);
    G16_TRY(raise_histogram_lds_limit());
    // unpadded bucket regions: second partition level + LDS-resident final level (4m above).  Sub-classes of 2^sublog
    // buckets, the largest size whose EXPECTED load leaves a quarter of the final level's LDS list free (2^6 at 2^22, c = 20); what
    // exceeds the list anyway is scattered directly by the same kernel.  Padded regions (G16_MSM_AFFINE_LEVELS > 0) keep the
    // histogram-matrix scatter, which places entries by `offsets`.
    const bool two_level = R == 0;
    uint32_t sublog = 0, S = 1;
    unsigned gx2 = 1;
    if (two_level) {
        const uint64_t mean_x4 = 4 * (nw / (uint64_t)plan.shard_n) / M + 1;   // 4 x the mean bucket load
        const uint32_t lo_log = slog > 8 ? slog - 8 : 0u;                     // S <= MAX_SUBS
        sublog = std::min<uint32_t>(slog, MAX_SUB_LOG);
        while (sublog > lo_log && (mean_x4 << sublog) > 3 * (uint64_t)FINAL_CAP) --sublog;
        if (sublog > MAX_SUB_LOG) return G16_ERR_INTERNAL;
        S = Bs >> sublog;
        // ~4096 workgroups of 256 lanes over the class regions, a tile of SUB_TILE entries at a time
        gx2 = std::max(1u, std::min(std::min(4096u / Q, 256u), (unsigned)((nw + SUB_TILE - 1) / SUB_TILE)));
    }
    const uint32_t sub_cells = two_level ? Q * S * gx2 : 0u;
    const uint32_t max_scan = std::max(std::max(M, Q * nb), sub_cells);
    G16_TRY(arena.alloc_n((size_t)(max_scan + SCAN_TILE - 1) / SCAN_TILE, &block_sums));
    auto prefix_scan = [&](const uint32_t* vals, uint32_t* prefix, uint32_t count) -> int {
        return prefix_scan_u32(vals, prefix, count, 0u, block_sums, st);
    };
    // ~4096 workgroups of 256 lanes over the class regions (a class region may hold anything between nothing and all
    // entries), at most 256 per class: every workgroup zeroes, stores and re-reads a histogram row whatever it counts
    unsigned gx = std::max(1u, std::min(std::min(4096u / Q, 256u), (unsigned)((nw + SORT_M_THREADS - 1) / SORT_M_THREADS)));
    if (const char* e = getenv("G16_SORT_GX")) {   // experiments: workgroups per class of the histogram-matrix scatter (padded regions)
        const int v = atoi(e);
        if (v >= 1 && v <= 4096) gx = (unsigned)v;
    }
    uint32_t* wg_counts = nullptr;   // padded regions: [class][workgroup][bucket] histograms, then their prefixes over the workgroups
    if (!two_level) G16_TRY(arena.alloc_n((size_t)Q * gx * Bs, &wg_counts));
    uint16_t* sub_key = nullptr;     // two-level plan: entry keys and tags, sub-class-partitioned
    uint32_t *sub_tag = nullptr, *sub_cnt = nullptr, *sub_off = nullptr;
    if (two_level) {
        G16_TRY(arena.alloc_n(nw ? nw : 1, &sub_key));
        G16_TRY(arena.alloc_n(nw ? nw : 1, &sub_tag));
        G16_TRY(arena.alloc_n((size_t)sub_cells + 1, &sub_cnt));
        G16_TRY(arena.alloc_n((size_t)sub_cells + 1, &sub_off));
    }
    if (n) {
        hipLaunchKernelGGL((class_count_kernel<Fr>), dim3(nb), dim3(CLASS_THREADS), 0, st, d_scalars, n, pd, slog, Q, class_cnt);
        G16_LAUNCH_CHECK();
        G16_TRY(prefix_scan(class_cnt, class_off, Q * nb));
        hipLaunchKernelGGL((class_partition_kernel<Fr>), dim3(nb), dim3(CLASS_THREADS), 0, st, d_scalars, n, pd, slog, Q, class_off, planes,
                           ent_tag);
        G16_LAUNCH_CHECK();
        if (two_level) {
            hipLaunchKernelGGL(sub_count_kernel, dim3(gx2, Q), dim3(SORT_M_THREADS), 0, st, planes, class_off, nb, S, sublog, sub_cnt);
            G16_LAUNCH_CHECK();
            G16_TRY(prefix_scan(sub_cnt, sub_off, sub_cells));
            hipLaunchKernelGGL(sub_partition_kernel, dim3(gx2, Q), dim3(SORT_M_THREADS), 0, st, planes, ent_tag, class_off, nb, S, sublog,
                               sub_off, sub_key, sub_tag);
            G16_LAUNCH_CHECK();
            // writes counts[] AND the sorted list: what follows only derives offsets, slots and the heavy list from the counts
            hipLaunchKernelGGL(final_sort_kernel, dim3(Q * S), dim3(SORT_M_THREADS), 0, st, sub_key, sub_tag, sub_off, gx2, sublog, counts,
                               out->sorted);
        } else {
            hipLaunchKernelGGL(bucket_count_merged_kernel, dim3(gx, Q), dim3(SORT_M_THREADS), lds, st, planes, class_off, nb, Bs,
                               wg_counts);
            G16_LAUNCH_CHECK();
            hipLaunchKernelGGL(bucket_wg_scan_kernel, dim3((M + 255) / 256), dim3(256), 0, st, wg_counts, gx, Bs, M, counts);
        }
        G16_LAUNCH_CHECK();
    }
    if (parts) G16_TRY(msm_parts_layout(counts, M, plan.Lmax, out->offsets, nparts, out->task_off, out->heavy, out->tasks, part_scratch, st));
    else G16_TRY(msm_slot_layout(counts, M, R, plan.Lmax, out->offsets, nparts, out->task_off, out->heavy, block_sums, st));
    if (n && !two_level) {
        hipLaunchKernelGGL(bucket_scatter_merged_kernel, dim3(gx, Q), dim3(SORT_M_THREADS), lds, st, planes, ent_tag, class_off, nb, Bs,
                           out->offsets, wg_counts, out->sorted);
        G16_LAUNCH_CHECK();
    }
    return G16_OK;
}

template int sort_scalars<Bls12_381>(const Bls12_381::Fr*, uint64_t, int, Arena&, hipStream_t, ScalarSort*, int, int, int);
template int sort_scalars<Bn254>(const Bn254::Fr*, uint64_t, int, Arena&, hipStream_t, ScalarSort*, int, int, int);

}  // namespace g16
