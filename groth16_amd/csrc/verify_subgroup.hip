// Prime-order subgroup membership for batches of points on the GPU: the tests of subgroup.hpp, one point per lane.
//
//   subgroup_g1_kernel / subgroup_g2_kernel   lane i of grid row g reads the affine point at base + g * group_stride + i * stride
//                              (64-bit words), runs the on-curve test and then the membership chain, and stores one byte at
//                              flags[g * n + i]: 1 member, 0 on the curve but outside the subgroup, 2 off the curve.  The strides
//                              let one launch walk a packed array (one row) or A and C of an n x (A | B | C) proof array (two
//                              rows, 6 L words apart) in place.  G1 and G2 are separate kernels: a wave never mixes Fq and Fq2
//                              chains.  No LDS, nothing shared between lanes.
//   subgroup_combine_kernel    the three point flags of a proof -> the proof's flag, and (for the checked aggregate verifier) one
//                              summary word per call: bit 0 some proof is outside a subgroup, bit 1 some point is off its curve.
// g16_host_check_subgroups runs the same templates on the CPU.
#include "subgroup.hpp"
#include "verify_common.hpp"

using namespace g16;

namespace g16 {

// Waves per SIMD the chains are compiled for.  A chain is one XYZZ accumulator and the base point: at 128 registers the BLS12-381
// kernels spill a few hundred bytes more than at 256 (G1 816 B against 224 B, G2 3.5 KB against 3.2 KB -- the out-of-line Fq2 products
// pass their operands in scratch either way) and twice the waves hide the multiply-add latency of the dependent field products.
constexpr int SUBGROUP_WAVES = 4;

template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, SUBGROUP_WAVES) void subgroup_g1_kernel(const uint64_t* base, uint64_t stride, uint64_t group_stride, uint64_t n,
                                                                   uint8_t* flags) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = blockIdx.y;
    flags[g * n + i] = Subgroup<C>::g1_flag(ld_any<typename C::G1A>(base + g * group_stride + i * stride));
}

template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, SUBGROUP_WAVES) void subgroup_g2_kernel(const uint64_t* base, uint64_t stride, uint64_t group_stride, uint64_t n,
                                                                   uint8_t* flags) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = blockIdx.y;
    flags[g * n + i] = Subgroup<C>::g2_flag(ld_any<typename C::G2A>(base + g * group_stride + i * stride));
}

// pt: flags of A (n), C (n), B (n); summary may be null
__global__ __launch_bounds__(256) void subgroup_combine_kernel(const uint8_t* pt, uint64_t n, uint8_t* flags, int* summary) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t f = subgroup_proof_flag(pt[i], pt[2 * n + i], pt[n + i]);
    flags[i] = f;
    if (summary && f != 1) atomicOr(summary, f == 2 ? 2 : 1);
}

template <class C>
int enqueue_points(hipStream_t s, int g2, const uint64_t* d_base, uint64_t stride, uint64_t group_stride, unsigned groups, uint64_t n,
                   uint8_t* d_flags) {
    const uint64_t blocks = (n + VERIFY_BLOCK - 1) / VERIFY_BLOCK;
    if (!n) return G16_OK;
    if (blocks > 0x7fffffffull) return G16_ERR_BAD_ARG;
    if (g2) subgroup_g2_kernel<C><<<dim3((unsigned)blocks, groups), VERIFY_BLOCK, 0, s>>>(d_base, stride, group_stride, n, d_flags);
    else subgroup_g1_kernel<C><<<dim3((unsigned)blocks, groups), VERIFY_BLOCK, 0, s>>>(d_base, stride, group_stride, n, d_flags);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

template <class C>
int enqueue_proofs(hipStream_t s, const uint64_t* d_proofs, uint64_t n, uint8_t* d_point_flags, uint8_t* d_flags, int* d_summary) {
    constexpr int L = C::Fq::N / 2;
    G16_TRY(enqueue_points<C>(s, 0, d_proofs, 8 * L, 6 * L, 2, n, d_point_flags));              // A -> [0, n), C -> [n, 2n)
    G16_TRY(enqueue_points<C>(s, 1, d_proofs + 2 * L, 8 * L, 0, 1, n, d_point_flags + 2 * n));   // B -> [2n, 3n)
    subgroup_combine_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_point_flags, n, d_flags, d_summary);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

int subgroup_enqueue_proofs(hipStream_t s, int curve, const uint64_t* d_proofs, uint64_t n, uint8_t* d_point_flags, uint8_t* d_flags,
                            int* d_summary) {
    if (curve == G16_BLS12_381) return enqueue_proofs<Bls12_381>(s, d_proofs, n, d_point_flags, d_flags, d_summary);
    if (curve == G16_BN254) return enqueue_proofs<Bn254>(s, d_proofs, n, d_point_flags, d_flags, d_summary);
    return G16_ERR_BAD_ARG;
}

int subgroup_enqueue_points(hipStream_t s, int curve, int g2, const uint64_t* d_points, uint64_t n, uint8_t* d_flags) {
    if (curve == G16_BLS12_381) return enqueue_points<Bls12_381>(s, g2, d_points, g2 ? 24 : 12, 0, 1, n, d_flags);
    if (curve == G16_BN254) return enqueue_points<Bn254>(s, g2, d_points, g2 ? 16 : 8, 0, 1, n, d_flags);
    return G16_ERR_BAD_ARG;
}

// items: packed points (words = 2 L or 4 L each) or whole proofs (proofs = true, 8 L words); one flag byte per item, in input order
template <class C>
int check_any(g16_ctx* ctx, bool proofs, int g2, const uint64_t* items, uint64_t n, uint8_t* flags) {
    constexpr int L = C::Fq::N / 2;
    const uint64_t words = proofs ? 8 * L : (g2 ? 4 * L : 2 * L);
    CtxView cv;
    G16_TRY(cv.load(ctx));
    if (cv.curve != C::CURVE_ID) return G16_ERR_BAD_ARG;
    return for_each_chunk(cv, n, [&](uint64_t k, uint64_t lo, uint64_t cnt, DevBufs& bufs) -> int {
        hipStream_t s = cv.streams[k];
        G16_HIP_TRY(hipSetDevice(cv.devs[k]));
        uint64_t* d_items;
        uint8_t *d_flags, *d_pt;
        G16_TRY(bufs.get(&d_items, cnt * words));
        G16_TRY(bufs.get(&d_flags, cnt));
        G16_HIP_TRY(hipMemcpyAsync(d_items, items + lo * words, cnt * words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        if (proofs) {
            G16_TRY(bufs.get(&d_pt, 3 * cnt));
            G16_TRY(enqueue_proofs<C>(s, d_items, cnt, d_pt, d_flags, nullptr));
        } else {
            G16_TRY(enqueue_points<C>(s, g2, d_items, words, 0, 1, cnt, d_flags));
        }
        G16_HIP_TRY(hipMemcpyAsync(flags + lo, d_flags, cnt, hipMemcpyDeviceToHost, s));
        return G16_OK;
    });
}

template <class C>
int host_check(int g2, const uint64_t* points, uint64_t n, uint8_t* flags) {
    constexpr int L = C::Fq::N / 2;
    for (uint64_t i = 0; i < n; ++i)
        flags[i] = g2 ? Subgroup<C>::g2_flag(ld_any<typename C::G2A>(points + i * 4 * L)) : Subgroup<C>::g1_flag(ld_any<typename C::G1A>(points + i * 2 * L));
    return G16_OK;
}

}  // namespace g16

extern "C" {

int g16_check_subgroups(g16_ctx* ctx, int g2, const uint64_t* points, uint64_t n, uint8_t* flags) {
    if (!ctx || (g2 != 0 && g2 != 1) || (n && (!points || !flags))) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(ctx_curve(ctx), (check_any<CC>(ctx, false, g2, points, n, flags)));
}

int g16_check_proof_subgroups(g16_ctx* ctx, const uint64_t* proofs, uint64_t n, uint8_t* flags) {
    if (!ctx || (n && (!proofs || !flags))) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(ctx_curve(ctx), (check_any<CC>(ctx, true, 0, proofs, n, flags)));
}

int g16_host_check_subgroups(int curve, int g2, const uint64_t* points, uint64_t n, uint8_t* flags) {
    if ((g2 != 0 && g2 != 1) || (n && (!points || !flags))) return G16_ERR_BAD_ARG;
    if (curve != G16_BLS12_381 && curve != G16_BN254) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(curve, (host_check<CC>(g2, points, n, flags)));
}

}  // extern "C"
