// Randomised batch verification of Groth16 proofs under one verifying key: one equation and one final exponentiation per batch.
//
// For coefficients r_1 .. r_n (128 bits, non-zero, drawn after the proofs are fixed) all n proofs hold iff, up to 2^-127,
//
//     FE( prod_i ML(r_i A_i, B_i) * ML(S_IC, -gamma) * ML(S_C, -delta) ) == e(alpha, beta)^s
//     s = sum r_i,  t_j = sum_i r_i x_ij,  S_IC = s gamma_abc[0] + sum_j t_j gamma_abc[j + 1],  S_C = sum r_i C_i.
//
//   verify_agg_miller_kernel   per proof: on-curve checks, r_i A_i and r_i C_i, the Miller loop over the one live pair
//                              (r_i A_i, B_i) without the final steps; the proofs of one lane share one accumulator (one Fq12
//                              squaring per loop step for all of them).  The 64 lanes of a workgroup (one wave) then multiply
//                              their f and add their r_i C_i through cross-lane moves, lane 0 writes the workgroup's pair.
//   verify_agg_reduce_kernel   the same wave reduction over 64 workgroup results at a time, until one pair is left.
//   verify_agg_scalar_kernel   s and the t_j in Fr: a grid column per j, partial sums per workgroup in LDS;
//   verify_agg_scalar_reduce_kernel  adds the partial sums.
//   (g16_verify_aggregate_checked runs the membership kernels of verify_subgroup.hip first, over the same uploaded proofs and on
//   the same stream: verdict 3 when a point is on its curve but outside its prime-order subgroup)
//   agg_key_tail, agg_finish   once per call, on the host templates (a lone GPU lane runs this chain about ten times slower than
//   (host)                     one host thread): S_IC, the two pairs with -gamma and -delta, finish_loop, ONE final
//                              exponentiation, and e(alpha, beta)^s as a cyclotomic power of the stored GT value -- chosen over a
//                              fourth pair (-s alpha, beta) because it needs nothing new in the prepared key and keeps the
//                              comparison the one verify_proof makes.
// g16_host_verify_aggregate runs the same per-proof function and the same tail on the CPU.
// The per-proof function (agg_terms), the wave reductions, the workgroup sum, the membership stage, the verdict precedence, the host
// tail and the chunk loop live in verify_common.hpp: verify_mixed.hip, the form for batches that mix verifying keys, uses them too.
#include "verify_common.hpp"
#include <cerrno>
#include <sys/random.h>

using namespace g16;

namespace g16 {

constexpr int AGG_SCALAR_BLOCK = 256;
constexpr int AGG_SCALAR_GRID = 64;   // workgroups per column of the scalar stage (at most)

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// lane g: proofs [g * per_lane, (g + 1) * per_lane); one (f, sc) per workgroup
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, 2) void verify_agg_miller_kernel(const uint64_t* proofs, const uint64_t* coeffs, uint64_t n,
                                                                          int per_lane, typename Pairing<C>::F12* f_out,
                                                                          XYZZ<typename Pairing<C>::F>* c_out, int* off_curve) {
    typedef Pairing<C> PP;
    constexpr int L = C::Fq::N / 2;
    const uint64_t lo = ((uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x) * (uint64_t)per_lane;
    const int cnt = lo < n ? (int)(n - lo < (uint64_t)per_lane ? n - lo : (uint64_t)per_lane) : 0;
    typename PP::F12 f = PP::F12::one();
    XYZZ<typename PP::F> sc = XYZZ<typename PP::F>::identity();
    if (cnt && !agg_terms<C>(proofs + lo * 8 * L, coeffs + lo * 2, cnt, f, sc)) {
        atomicOr(off_curve, 1);
        f = PP::F12::one();
        sc = XYZZ<typename PP::F>::identity();
    }
    wave_reduce<C>(f, sc);
    if (threadIdx.x == 0) {
        f_out[blockIdx.x] = f;
        c_out[blockIdx.x] = sc;
    }
}

// m pairs in, ceil(m / 64) out
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, 2) void verify_agg_reduce_kernel(const typename Pairing<C>::F12* f_in,
                                                                          const XYZZ<typename Pairing<C>::F>* c_in, uint64_t m,
                                                                          typename Pairing<C>::F12* f_out,
                                                                          XYZZ<typename Pairing<C>::F>* c_out) {
    typedef Pairing<C> PP;
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    typename PP::F12 f = PP::F12::one();
    XYZZ<typename PP::F> sc = XYZZ<typename PP::F>::identity();
    if (i < m) {
        f = f_in[i];
        sc = c_in[i];
    }
    wave_reduce<C>(f, sc);
    if (threadIdx.x == 0) {
        f_out[blockIdx.x] = f;
        c_out[blockIdx.x] = sc;
    }
}

// column j = blockIdx.y: j = 0 sums the r_i, j > 0 the r_i x_i(j-1); partial[blockIdx.x * (num_public + 1) + j]
template <class C>
__global__ __launch_bounds__(AGG_SCALAR_BLOCK) void verify_agg_scalar_kernel(const uint64_t* coeffs, const uint64_t* inputs,
                                                                              uint64_t num_public, uint64_t n, typename C::Fr* partial) {
    typedef typename C::Fr Fr;
    __shared__ Fr sh[AGG_SCALAR_BLOCK];
    const uint64_t j = blockIdx.y;
    const Fr* x = reinterpret_cast<const Fr*>(inputs);
    Fr acc = Fr::zero();
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_SCALAR_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * AGG_SCALAR_BLOCK) {
        const Fr r = coeff_fr<Fr>(coeffs + 2 * i);
        acc = acc + (j ? r * x[i * num_public + (j - 1)] : r);
    }
    const Fr sum = agg_block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(uint64_t)blockIdx.x * (num_public + 1) + j] = sum;
}

// out[j] = sum_b partial[b * cols + j], one workgroup per column
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK) void verify_agg_scalar_reduce_kernel(const typename C::Fr* partial, uint64_t rows, uint64_t cols,
                                                                                 typename C::Fr* out) {
    typedef typename C::Fr Fr;
    __shared__ Fr sh[VERIFY_BLOCK];
    Fr acc = Fr::zero();
    for (uint64_t b = threadIdx.x; b < rows; b += VERIFY_BLOCK) acc = acc + partial[b * cols + blockIdx.x];
    const Fr sum = agg_block_sum(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// the caller's coefficients (none may be zero) or fresh ones from the operating system's generator
int agg_coeffs(const uint64_t* coeffs, uint64_t n, std::vector<uint64_t>& own, const uint64_t** out) {
    if (coeffs) {
        for (uint64_t i = 0; i < n; ++i)
            if (!(coeffs[2 * i] | coeffs[2 * i + 1])) return G16_ERR_BAD_ARG;
        *out = coeffs;
        return G16_OK;
    }
    own.resize(2 * n);
    auto fill = [](void* p, size_t bytes) {
        uint8_t* b = static_cast<uint8_t*>(p);
        while (bytes) {
            const ssize_t got = getrandom(b, bytes, 0);
            if (got < 0) {
                if (errno == EINTR) continue;
                return false;
            }
            b += got;
            bytes -= (size_t)got;
        }
        return true;
    };
    if (!fill(own.data(), 2 * n * sizeof(uint64_t))) return G16_ERR_INTERNAL;
    for (uint64_t i = 0; i < n; ++i)
        while (!(own[2 * i] | own[2 * i + 1]))
            if (!fill(&own[2 * i], 2 * sizeof(uint64_t))) return G16_ERR_INTERNAL;
    *out = own.data();
    return G16_OK;
}

template <class C>
int host_verify_aggregate(const g16_vk_view* vk, const uint64_t* proofs, uint64_t n, const uint64_t* inputs, uint64_t num_public,
                          const uint64_t* coeffs, uint8_t* verdict, uint64_t* lhs_out, uint64_t* rhs_out) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    typedef typename C::Fr Fr;
    constexpr int L = C::Fq::N / 2;
    std::vector<uint64_t> own;
    const uint64_t* r = nullptr;
    G16_TRY(agg_coeffs(coeffs, n, own, &r));
    typename PP::F12 f = PP::F12::one();
    XYZZ<F> sc = XYZZ<F>::identity();
    std::vector<Fr> st(num_public + 1, Fr::zero());
    bool on_curve = true;
    for (uint64_t i = 0; i < n; i += AGG_MAX_PER_LANE) {   // in groups that share an accumulator, as the lanes of the kernel do
        typename PP::F12 fi;
        XYZZ<F> ci;
        if (!agg_terms<C>(proofs + i * 8 * L, r + 2 * i, (int)std::min<uint64_t>(AGG_MAX_PER_LANE, n - i), fi, ci)) { on_curve = false; continue; }
        f = f * fi;
        sc.add(ci);
    }
    for (uint64_t i = 0; i < n; ++i) {
        const Fr ri = coeff_fr<Fr>(r + 2 * i);
        st[0] = st[0] + ri;
        for (uint64_t j = 0; j < num_public; ++j) st[j + 1] = st[j + 1] + ri * ld<Fr>(inputs + (i * num_public + j) * 4);
    }
    if (!on_curve) {
        if (lhs_out) return G16_ERR_BAD_ARG;
        *verdict = 2;
        return G16_OK;
    }
    typename PP::F12 ab, g, rhs;
    G16_TRY(host_alpha_beta<C>(vk, ab));
    agg_key_tail<C>(sc, st.data(), num_public + 1, vk->gamma_g2, vk->delta_g2, vk->gamma_abc_g1, ab, g, rhs);
    return agg_finish<C>(f, g, rhs, verdict, lhs_out, rhs_out);
}

// ---- device side of g16_verify_aggregate ---------------------------------------------------------------------------------------
template <class C>
struct AggPartial {   // what one device hands back
    typename Pairing<C>::F12 f;
    XYZZ<typename Pairing<C>::F> sc;
    std::vector<typename C::Fr> st;
    int off_curve = 0;
    int off_subgroup = 0;   // the membership stage's summary (checked calls): bit 0 outside a subgroup, bit 1 off a curve
    int undecodable = 0;    // the decoding stage's summary (byte input): bit 0 some proof's bytes do not decode
};

// Proofs per lane.  Sharing an accumulator saves a lane work but lengthens its chain, so it pays only while every SIMD keeps its two
// waves: m proofs share a lane once the batch fills the resident lanes m times over.  Measured on one MI355X (131072 resident lanes),
// BLS12-381: 2^17 proofs at one per lane 88.4 ms, 2^17 + 64 at two per lane (half the waves) 96.0 ms, 2^18 at two per lane 146.7 ms.
inline int agg_per_lane(int device, uint64_t n) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    const uint64_t resident = (uint64_t)cus * 4 * 2 * VERIFY_BLOCK;
    return (int)std::min<uint64_t>(std::max<uint64_t>(n / resident, 1), AGG_MAX_PER_LANE);
}

// The byte input of g16_verify_aggregate_bytes: uploads n compressed proofs (a third of the affine form), decodes them into a device
// buffer on the same stream and hands that buffer to aggregate_chunk; an undecodable point is the identity there.
template <class C>
int decode_chunk(hipStream_t s, int device, const uint8_t* bytes, uint64_t n, AggPartial<C>* out, DevBufs& bufs, uint64_t** d_resident) {
    constexpr int L = C::Fq::N / 2;
    constexpr uint64_t PROOF_BYTES = 4 * ((C::Fq::Params::BITS + 7) / 8);
    G16_HIP_TRY(hipSetDevice(device));
    uint8_t *d_bytes, *d_pt, *d_status;
    int* d_bad;
    G16_TRY(bufs.get(&d_bytes, n * PROOF_BYTES));
    G16_TRY(bufs.get(d_resident, n * 8 * L));
    G16_TRY(bufs.get(&d_pt, 3 * n));
    G16_TRY(bufs.get(&d_status, n));
    G16_TRY(bufs.get(&d_bad, 1));
    G16_HIP_TRY(hipMemcpyAsync(d_bytes, bytes, n * PROOF_BYTES, hipMemcpyHostToDevice, s));
    G16_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), s));
    G16_TRY(decompress_enqueue_proofs(s, C::CURVE_ID, d_bytes, n, *d_resident, d_pt, d_status, d_bad));
    G16_HIP_TRY(hipMemcpyAsync(&out->undecodable, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
    return G16_OK;
}

// proofs: n x (A | B | C) affine in host memory, uploaded here -- or d_resident: the same already on this device (written by earlier
// work on s)
template <class C>
int aggregate_chunk(hipStream_t s, int device, const uint64_t* proofs, const uint64_t* d_resident, const uint64_t* inputs, uint64_t num_public,
                    const uint64_t* coeffs, uint64_t n, bool check, AggPartial<C>* out, DevBufs& bufs) {
    typedef Pairing<C> PP;
    typedef XYZZ<typename PP::F> G1X;
    typedef typename C::Fr Fr;
    constexpr int L = C::Fq::N / 2;
    G16_HIP_TRY(hipSetDevice(device));
    const int per_lane = agg_per_lane(device, n);
    const uint64_t lanes = (n + per_lane - 1) / per_lane;
    const uint64_t blocks = (lanes + VERIFY_BLOCK - 1) / VERIFY_BLOCK, blocks2 = (blocks + VERIFY_BLOCK - 1) / VERIFY_BLOCK;
    const unsigned sgrid = (unsigned)std::min<uint64_t>((n + AGG_SCALAR_BLOCK - 1) / AGG_SCALAR_BLOCK, AGG_SCALAR_GRID);
    const uint64_t cols = num_public + 1;
    const uint64_t* d_proofs = d_resident;
    uint64_t *d_upload, *d_coeffs, *d_inputs;
    typename PP::F12* d_f[2];
    G1X* d_c[2];
    Fr *d_part, *d_st;
    int* d_off;
    if (!d_resident) {
        G16_TRY(bufs.get(&d_upload, n * 8 * L));
        d_proofs = d_upload;
    }
    G16_TRY(bufs.get(&d_coeffs, n * 2));
    G16_TRY(bufs.get(&d_inputs, n * num_public * 4));
    G16_TRY(bufs.get(&d_f[0], blocks));
    G16_TRY(bufs.get(&d_f[1], blocks2));
    G16_TRY(bufs.get(&d_c[0], blocks));
    G16_TRY(bufs.get(&d_c[1], blocks2));
    G16_TRY(bufs.get(&d_part, sgrid * cols));
    G16_TRY(bufs.get(&d_st, cols));
    G16_TRY(bufs.get(&d_off, 1));
    if (!d_resident) G16_HIP_TRY(hipMemcpyAsync(d_upload, proofs, n * 8 * L * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    G16_HIP_TRY(hipMemcpyAsync(d_coeffs, coeffs, n * 2 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (num_public) G16_HIP_TRY(hipMemcpyAsync(d_inputs, inputs, n * num_public * 4 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    G16_HIP_TRY(hipMemsetAsync(d_off, 0, sizeof(int), s));
    if (check) G16_TRY(agg_membership_enqueue(s, C::CURVE_ID, d_proofs, n, bufs, &out->off_subgroup));
    verify_agg_scalar_kernel<C><<<dim3(sgrid, (unsigned)cols), AGG_SCALAR_BLOCK, 0, s>>>(d_coeffs, d_inputs, num_public, n, d_part);
    G16_LAUNCH_CHECK();
    verify_agg_scalar_reduce_kernel<C><<<(unsigned)cols, VERIFY_BLOCK, 0, s>>>(d_part, sgrid, cols, d_st);
    G16_LAUNCH_CHECK();
    verify_agg_miller_kernel<C><<<(unsigned)blocks, VERIFY_BLOCK, 0, s>>>(d_proofs, d_coeffs, n, per_lane, d_f[0], d_c[0], d_off);
    G16_LAUNCH_CHECK();
    int cur = 0;
    for (uint64_t m = blocks; m > 1; m = (m + VERIFY_BLOCK - 1) / VERIFY_BLOCK, cur ^= 1) {
        verify_agg_reduce_kernel<C><<<(unsigned)((m + VERIFY_BLOCK - 1) / VERIFY_BLOCK), VERIFY_BLOCK, 0, s>>>(d_f[cur], d_c[cur], m, d_f[cur ^ 1],
                                                                                                               d_c[cur ^ 1]);
        G16_LAUNCH_CHECK();
    }
    out->st.resize(cols);
    G16_HIP_TRY(hipMemcpyAsync(&out->f, d_f[cur], sizeof(out->f), hipMemcpyDeviceToHost, s));
    G16_HIP_TRY(hipMemcpyAsync(&out->sc, d_c[cur], sizeof(out->sc), hipMemcpyDeviceToHost, s));
    G16_HIP_TRY(hipMemcpyAsync(out->st.data(), d_st, cols * sizeof(Fr), hipMemcpyDeviceToHost, s));
    G16_HIP_TRY(hipMemcpyAsync(&out->off_curve, d_off, sizeof(int), hipMemcpyDeviceToHost, s));
    return G16_OK;
}

// proofs (affine) or bytes (compressed, decoded on the device; check is then set)
template <class C>
int aggregate_any(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, const uint8_t* bytes, uint64_t n, const uint64_t* inputs,
                  uint64_t num_public, const uint64_t* coeffs, bool check, uint8_t* verdict) {
    typedef Pairing<C> PP;
    constexpr int L = C::Fq::N / 2;
    constexpr uint64_t PROOF_BYTES = 4 * ((C::Fq::Params::BITS + 7) / 8);
    std::vector<uint64_t> own;
    const uint64_t* r = nullptr;
    G16_TRY(agg_coeffs(coeffs, n, own, &r));
    CtxView cv;
    G16_TRY(cv.load(ctx));
    const uint64_t nd = cv.devs.size();
    if (devs_of<C>(const_cast<g16_pvk*>(pvk)).size() != nd) return G16_ERR_BAD_ARG;   // the key was loaded on another context
    std::vector<AggPartial<C>> part(nd);
    std::vector<char> used(nd, 0);   // an empty chunk contributes nothing to the product
    const int rc = for_each_chunk(cv, n, [&](uint64_t k, uint64_t lo, uint64_t cnt, DevBufs& bufs) -> int {
        used[k] = 1;
        uint64_t* d_resident = nullptr;
        if (bytes) G16_TRY(decode_chunk<C>(cv.streams[k], cv.devs[k], bytes + lo * PROOF_BYTES, cnt, &part[k], bufs, &d_resident));
        return aggregate_chunk<C>(cv.streams[k], cv.devs[k], bytes ? nullptr : proofs + lo * 8 * L, d_resident,
                                  inputs ? inputs + lo * num_public * 4 : nullptr, num_public, r + 2 * lo, cnt, check, &part[k], bufs);
    });
    if (rc != G16_OK) return rc;
    typename PP::F12 f = PP::F12::one();
    XYZZ<typename PP::F> sc = XYZZ<typename PP::F>::identity();
    std::vector<typename C::Fr> st(num_public + 1, C::Fr::zero());
    int off_curve = 0, off_subgroup = 0, undecodable = 0;
    for (uint64_t k = 0; k < nd; ++k) {
        if (!used[k]) continue;
        f = f * part[k].f;
        sc.add(part[k].sc);
        for (uint64_t j = 0; j <= num_public; ++j) st[j] = st[j] + part[k].st[j];
        off_curve |= part[k].off_curve;
        off_subgroup |= part[k].off_subgroup;
        undecodable |= part[k].undecodable;
    }
    if (const uint8_t v = agg_early_verdict(undecodable, off_curve, off_subgroup)) { *verdict = v; return G16_OK; }
    typename PP::F12 g, rhs;
    agg_key_tail<C>(sc, st.data(), num_public + 1, pvk->gamma_g2.data(), pvk->delta_g2.data(), pvk->gamma_abc_g1.data(), PP::load_gt(pvk->ab), g,
                    rhs);
    return agg_finish<C>(f, g, rhs, verdict, nullptr, nullptr);
}

int aggregate_call(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, const uint8_t* bytes, uint64_t n, const uint64_t* inputs,
                   uint64_t num_public, const uint64_t* coeffs, bool check, uint8_t* verdict) {
    if (!ctx || !pvk || !verdict || (n && !proofs && !bytes) || (n && num_public && !inputs)) return G16_ERR_BAD_ARG;
    if (num_public + 1 != pvk->n_gamma_abc) return G16_ERR_MALFORMED_VK;
    if (!n) { *verdict = 1; return G16_OK; }
    G16_VERIFY_DISPATCH(pvk->curve, (aggregate_any<CC>(ctx, pvk, proofs, bytes, n, inputs, num_public, coeffs, check, verdict)));
}

}  // namespace g16

extern "C" {

int g16_verify_aggregate(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                         uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict) {
    return aggregate_call(ctx, pvk, proofs, nullptr, n, public_inputs, num_public, coeffs, false, verdict);
}

int g16_verify_aggregate_checked(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                                 uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict) {
    return aggregate_call(ctx, pvk, proofs, nullptr, n, public_inputs, num_public, coeffs, true, verdict);
}

int g16_host_verify_aggregate(int curve, const g16_vk_view* vk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                              uint64_t num_public, const uint64_t* coeffs, uint8_t* verdict) {
    if (!vk_view_ok(vk) || !verdict || (n && !proofs) || (n && num_public && !public_inputs)) return G16_ERR_BAD_ARG;
    if (num_public + 1 != vk->n_gamma_abc) return G16_ERR_MALFORMED_VK;
    if (curve != G16_BLS12_381 && curve != G16_BN254) return G16_ERR_BAD_ARG;
    if (!n) { *verdict = 1; return G16_OK; }
    G16_VERIFY_DISPATCH(curve, (host_verify_aggregate<CC>(vk, proofs, n, public_inputs, num_public, coeffs, verdict, nullptr, nullptr)));
}

int g16_host_verify_aggregate_gt(int curve, const g16_vk_view* vk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                                 uint64_t num_public, const uint64_t* coeffs, uint64_t* lhs_fq12, uint64_t* rhs_fq12) {
    if (!vk_view_ok(vk) || !lhs_fq12 || !rhs_fq12 || !coeffs || !n || !proofs || (num_public && !public_inputs)) return G16_ERR_BAD_ARG;
    if (num_public + 1 != vk->n_gamma_abc) return G16_ERR_MALFORMED_VK;
    G16_VERIFY_DISPATCH(curve, (host_verify_aggregate<CC>(vk, proofs, n, public_inputs, num_public, coeffs, nullptr, lhs_fq12, rhs_fq12)));
}

}  // extern "C"
