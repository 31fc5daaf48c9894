// Compressed points and proofs decoded on the GPU: the templates of decompress.hpp, one point per lane.
//
//   decompress_g1_kernel / decompress_g2_kernel   lane i of grid row g reads the encoding at in + g * in_group + i * in_stride (bytes),
//                              takes the square root and stores the affine point at out + g * out_group + i * out_stride (64-bit
//                              words) and one byte at status[g * n + i]: 1 decoded, 0 not (the identity is stored then, so no later
//                              kernel reads undefined memory).  The strides let one launch walk a packed array (one row) or A and C
//                              of a proof array (two rows) from A | B | C bytes into A | B | C limbs.  G1 and G2 are separate
//                              kernels: a wave never mixes Fq and Fq2 chains.  No LDS, nothing shared between lanes.
//   decompress_combine_kernel  the three point statuses of a proof -> the proof's status, and (for g16_verify_aggregate_bytes) one
//                              summary word per call: bit 0 some proof does not decode.
// g16_host_decompress_points runs the same templates on the CPU.
#include "decompress.hpp"
#include "verify_common.hpp"

using namespace g16;

namespace g16 {

// Waves per SIMD the chains are compiled for: a lane holds the running power, the base and one product's temporaries, which fit 128
// registers; the dependent squarings of one lane leave the multiplier idle between them, so more waves hide more of that latency.
constexpr int DECOMPRESS_WAVES = 4;

template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, DECOMPRESS_WAVES) void decompress_g1_kernel(const uint8_t* in, uint64_t in_stride, uint64_t in_group,
                                                                                       uint64_t* out, uint64_t out_stride, uint64_t out_group,
                                                                                       uint64_t n, uint8_t* status) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = blockIdx.y;
    typename C::G1A p;
    status[g * n + i] = Decompress<C>::g1(in + g * in_group + i * in_stride, &p);
    __builtin_memcpy(out + g * out_group + i * out_stride, &p, sizeof(p));
}

template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, DECOMPRESS_WAVES) void decompress_g2_kernel(const uint8_t* in, uint64_t in_stride, uint64_t in_group,
                                                                                       uint64_t* out, uint64_t out_stride, uint64_t out_group,
                                                                                       uint64_t n, uint8_t* status) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = blockIdx.y;
    typename C::G2A p;
    status[g * n + i] = Decompress<C>::g2(in + g * in_group + i * in_stride, &p);
    __builtin_memcpy(out + g * out_group + i * out_stride, &p, sizeof(p));
}

// pt: statuses of A (n), C (n), B (n); summary may be null
__global__ __launch_bounds__(256) void decompress_combine_kernel(const uint8_t* pt, uint64_t n, uint8_t* status, int* summary) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t f = decompress_proof_status(pt[i], pt[2 * n + i], pt[n + i]);
    status[i] = f;
    if (summary && f != 1) atomicOr(summary, 1);
}

template <class C>
int enqueue_decode_points(hipStream_t s, int g2, const uint8_t* d_in, uint64_t in_stride, uint64_t in_group, uint64_t* d_out,
                          uint64_t out_stride, uint64_t out_group, unsigned groups, uint64_t n, uint8_t* d_status) {
    const uint64_t blocks = (n + VERIFY_BLOCK - 1) / VERIFY_BLOCK;
    if (!n) return G16_OK;
    if (blocks > 0x7fffffffull) return G16_ERR_BAD_ARG;
    if (g2)
        decompress_g2_kernel<C><<<dim3((unsigned)blocks, groups), VERIFY_BLOCK, 0, s>>>(d_in, in_stride, in_group, d_out, out_stride, out_group, n,
                                                                                        d_status);
    else
        decompress_g1_kernel<C><<<dim3((unsigned)blocks, groups), VERIFY_BLOCK, 0, s>>>(d_in, in_stride, in_group, d_out, out_stride, out_group, n,
                                                                                        d_status);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

template <class C>
int enqueue_decode_proofs(hipStream_t s, const uint8_t* d_bytes, uint64_t n, uint64_t* d_proofs, uint8_t* d_point_status, uint8_t* d_status,
                          int* d_summary) {
    constexpr int L = C::Fq::N / 2;
    constexpr uint64_t FB = Decompress<C>::FQ_BYTES;
    G16_TRY(enqueue_decode_points<C>(s, 0, d_bytes, 4 * FB, 3 * FB, d_proofs, 8 * L, 6 * L, 2, n, d_point_status));   // A -> [0, n), C -> [n, 2n)
    G16_TRY(enqueue_decode_points<C>(s, 1, d_bytes + FB, 4 * FB, 0, d_proofs + 2 * L, 8 * L, 0, 1, n, d_point_status + 2 * n));   // B -> [2n, 3n)
    decompress_combine_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_point_status, n, d_status, d_summary);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

int decompress_enqueue_proofs(hipStream_t s, int curve, const uint8_t* d_bytes, uint64_t n, uint64_t* d_proofs, uint8_t* d_point_status,
                              uint8_t* d_status, int* d_summary) {
    if (curve == G16_BLS12_381) return enqueue_decode_proofs<Bls12_381>(s, d_bytes, n, d_proofs, d_point_status, d_status, d_summary);
    if (curve == G16_BN254) return enqueue_decode_proofs<Bn254>(s, d_bytes, n, d_proofs, d_point_status, d_status, d_summary);
    return G16_ERR_BAD_ARG;
}

template <class C>
int enqueue_decode_packed(hipStream_t s, int g2, const uint8_t* d_bytes, uint64_t n, uint64_t* d_points, uint8_t* d_status) {
    constexpr int L = C::Fq::N / 2;
    constexpr uint64_t FB = Decompress<C>::FQ_BYTES;
    return enqueue_decode_points<C>(s, g2, d_bytes, g2 ? 2 * FB : FB, 0, d_points, g2 ? 4 * L : 2 * L, 0, 1, n, d_status);
}

int decompress_enqueue_points(hipStream_t s, int curve, int g2, const uint8_t* d_bytes, uint64_t n, uint64_t* d_points, uint8_t* d_status) {
    if (curve == G16_BLS12_381) return enqueue_decode_packed<Bls12_381>(s, g2, d_bytes, n, d_points, d_status);
    if (curve == G16_BN254) return enqueue_decode_packed<Bn254>(s, g2, d_bytes, n, d_points, d_status);
    return G16_ERR_BAD_ARG;
}

// items: packed encodings (G1 or G2) or whole proofs (proofs = true); per item the affine form and one status byte, in input order
template <class C>
int decode_any(g16_ctx* ctx, bool proofs, int g2, const uint8_t* bytes, uint64_t n, uint64_t* out, uint8_t* status) {
    constexpr int L = C::Fq::N / 2;
    constexpr uint64_t FB = Decompress<C>::FQ_BYTES;
    const uint64_t in_sz = proofs ? 4 * FB : (g2 ? 2 * FB : FB), words = proofs ? 8 * L : (g2 ? 4 * L : 2 * L);
    CtxView cv;
    G16_TRY(cv.load(ctx));
    if (cv.curve != C::CURVE_ID) return G16_ERR_BAD_ARG;
    return for_each_chunk(cv, n, [&](uint64_t k, uint64_t lo, uint64_t cnt, DevBufs& bufs) -> int {
        hipStream_t s = cv.streams[k];
        G16_HIP_TRY(hipSetDevice(cv.devs[k]));
        uint8_t *d_in, *d_status, *d_pt;
        uint64_t* d_out;
        G16_TRY(bufs.get(&d_in, cnt * in_sz));
        G16_TRY(bufs.get(&d_out, cnt * words));
        G16_TRY(bufs.get(&d_status, cnt));
        G16_HIP_TRY(hipMemcpyAsync(d_in, bytes + lo * in_sz, cnt * in_sz, hipMemcpyHostToDevice, s));
        if (proofs) {
            G16_TRY(bufs.get(&d_pt, 3 * cnt));
            G16_TRY(enqueue_decode_proofs<C>(s, d_in, cnt, d_out, d_pt, d_status, nullptr));
        } else {
            G16_TRY(enqueue_decode_points<C>(s, g2, d_in, in_sz, 0, d_out, words, 0, 1, cnt, d_status));
        }
        G16_HIP_TRY(hipMemcpyAsync(out + lo * words, d_out, cnt * words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        G16_HIP_TRY(hipMemcpyAsync(status + lo, d_status, cnt, hipMemcpyDeviceToHost, s));
        return G16_OK;
    });
}

template <class C>
int host_decode(int g2, const uint8_t* bytes, uint64_t n, uint64_t* out, uint8_t* status) {
    constexpr int L = C::Fq::N / 2;
    typedef Decompress<C> D;
    for (uint64_t i = 0; i < n; ++i) {
        if (g2) {
            typename C::G2A p;
            status[i] = D::g2(bytes + i * D::G2_BYTES, &p);
            memcpy(out + i * 4 * L, &p, sizeof(p));
        } else {
            typename C::G1A p;
            status[i] = D::g1(bytes + i * D::G1_BYTES, &p);
            memcpy(out + i * 2 * L, &p, sizeof(p));
        }
    }
    return G16_OK;
}

}  // namespace g16

extern "C" {

int g16_decompress_points(g16_ctx* ctx, int g2, const uint8_t* bytes, uint64_t n, uint64_t* points_out, uint8_t* status) {
    if (!ctx || (g2 != 0 && g2 != 1) || (n && (!bytes || !points_out || !status))) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(ctx_curve(ctx), (decode_any<CC>(ctx, false, g2, bytes, n, points_out, status)));
}

int g16_decompress_proofs(g16_ctx* ctx, const uint8_t* bytes, uint64_t n, uint64_t* proofs_out, uint8_t* status) {
    if (!ctx || (n && (!bytes || !proofs_out || !status))) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(ctx_curve(ctx), (decode_any<CC>(ctx, true, 0, bytes, n, proofs_out, status)));
}

int g16_host_decompress_points(int curve, int g2, const uint8_t* bytes, uint64_t n, uint64_t* points_out, uint8_t* status) {
    if ((g2 != 0 && g2 != 1) || (n && (!bytes || !points_out || !status))) return G16_ERR_BAD_ARG;
    if (curve != G16_BLS12_381 && curve != G16_BN254) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(curve, (host_decode<CC>(g2, bytes, n, points_out, status)));
}

int g16_verify_aggregate_bytes(g16_ctx* ctx, const g16_pvk* pvk, const uint8_t* proof_bytes, uint64_t n, const uint64_t* public_inputs,
                               uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict) {
    return aggregate_call(ctx, pvk, nullptr, proof_bytes, n, public_inputs, num_public, coeffs, true, verdict);
}

}  // extern "C"
