// The three-launch exclusive prefix sum of msm.hip (step 3) as a header: the kernels are `static`, so each library that includes it
// carries its own copy -- the product library (msm.hip) and the part-walk library (partwalk.hip), which scans its length matrix.
#pragma once
#include "hd.hpp"
#include <cstdint>

namespace g16 {

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

}  // namespace g16
