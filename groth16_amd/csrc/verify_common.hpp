// What the five verify files share.  For all of them: a context's devices and streams, the chunk loop of a multi-device context, the
// device buffers of one call and the curve dispatch of the entry points.  For verify.hip (one verify_proof per lane),
// verify_aggregate.hip (one equation per batch under one key) and verify_mixed.hip (one equation per batch that mixes keys): the
// prepared key and its per-device part, the window-table form of prepare_inputs, the Miller loop on prepared lines, e(alpha, beta) on
// the host; for the two aggregate forms also the per-proof stage, the wave / workgroup reductions, the membership stage, the verdict
// precedence and the once-per-batch host tail.
#pragma once
#include "internal.hpp"
#include "pairing.hpp"
#include <algorithm>
#include <new>
#include <vector>

namespace g16 {
int ctx_devices(const g16_ctx* ctx, int* curve, std::vector<int>& devs, std::vector<hipStream_t>& streams);   // api.hip

// verify_subgroup.hip: enqueue the membership tests over n proofs (A | B | C) resident on the current device.  d_point_flags: 3 n
// bytes of work space, d_flags: one byte per proof (1 / 0 / 2 as g16_check_proof_subgroups), *d_summary (may be null, zeroed by the
// caller) |= 1 if a proof is outside a subgroup, 2 if a point is off its curve.
int subgroup_enqueue_proofs(hipStream_t s, int curve, const uint64_t* d_proofs, uint64_t n, uint8_t* d_point_flags, uint8_t* d_flags,
                            int* d_summary);

// verify_decompress.hip: enqueue the decoding of n compressed proofs (A | B | C bytes, resident on the current device) into d_proofs
// (n x (A | B | C) affine; a point that does not decode is written as the identity).  d_point_status: 3 n bytes of work space,
// d_status: one byte per proof (1 / 0 as g16_decompress_proofs), *d_summary (may be null, zeroed by the caller) |= 1 if a proof does
// not decode.
int decompress_enqueue_proofs(hipStream_t s, int curve, const uint8_t* d_bytes, uint64_t n, uint64_t* d_proofs, uint8_t* d_point_status,
                              uint8_t* d_status, int* d_summary);
// The same two stages over n PACKED points of one group resident on the current device (key_bytes.hip: a proving key's queries): the
// launches of g16_decompress_points / g16_check_subgroups without their uploads.  d_bytes: n compressed encodings, d_points: n affine
// points (written by the first, read by the second), d_status / d_flags: one byte per point as those calls give it.
int decompress_enqueue_points(hipStream_t s, int curve, int g2, const uint8_t* d_bytes, uint64_t n, uint64_t* d_points, uint8_t* d_status);
int subgroup_enqueue_points(hipStream_t s, int curve, int g2, const uint64_t* d_points, uint64_t n, uint8_t* d_flags);
// verify_aggregate.hip: the three single-key aggregate entry points, argument checks and the empty-batch rule included.  proofs
// (affine) or bytes (compressed, decoded on the device; check must then be set), the other null
int aggregate_call(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, const uint8_t* bytes, uint64_t n, const uint64_t* inputs,
                   uint64_t num_public, const uint64_t* coeffs, bool check, uint8_t* verdict);

constexpr int VERIFY_BLOCK = 64;

// host reads of caller memory: the point / field structs are 16-byte aligned, a caller's u64 buffer need not be
template <class T>
T ld(const void* p) {
    T t;
    memcpy(&t, p, sizeof(T));
    return t;
}
template <class T>
G16_HD T ld_any(const uint64_t* p) {   // caller memory on the host, 8-byte aligned words on the device
    T t;
    __builtin_memcpy(&t, p, sizeof(T));
    return t;
}

// device buffers of one call, freed together (on the device that is current then)
struct DevBufs {
    std::vector<void*> p;
    DevBufs() = default;
    DevBufs(const DevBufs&) = delete;
    ~DevBufs() { release(); }
    template <class T>
    int get(T** out, size_t count) {
        void* q = nullptr;
        G16_HIP_TRY(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
        p.push_back(q);
        *out = static_cast<T*>(q);
        return G16_OK;
    }
    void release() {
        for (void* q : p) (void)hipFree(q);
        p.clear();
    }
};

// a context's curve, and its devices with their streams: one entry, or one per device of a multi-device context
struct CtxView {
    int curve = -1;
    std::vector<int> devs;
    std::vector<hipStream_t> streams;
    int load(const g16_ctx* ctx) { return ctx_devices(ctx, &curve, devs, streams); }
};

inline int ctx_curve(const g16_ctx* ctx) {   // -1: no context
    CtxView cv;
    return cv.load(ctx) == G16_OK ? cv.curve : -1;
}

// The multi-device policy of every batch entry point: equal chunks of the n items, one per device of the context, all enqueued before
// any wait.  enqueue(k, lo, cnt, bufs) queues items [lo, lo + cnt), cnt >= 1, on device k (it selects the device itself) and takes its
// device memory from bufs.  Nothing more is enqueued after the first error; then every stream is waited for and every chunk's memory
// freed.  Returns the first error: a failed wait counts (G16_ERR_HIP) only if nothing failed before it.
template <class Enqueue>
int for_each_chunk(const CtxView& cv, uint64_t n, Enqueue&& enqueue) {
    const uint64_t nd = cv.devs.size();
    std::vector<DevBufs> bufs(nd);
    int rc = G16_OK;
    for (uint64_t k = 0; k < nd && rc == G16_OK; ++k) {
        const uint64_t lo = n * k / nd, hi = n * (k + 1) / nd;
        if (hi > lo) rc = enqueue(k, lo, hi - lo, bufs[k]);
    }
    for (uint64_t k = 0; k < nd; ++k) {
        (void)hipSetDevice(cv.devs[k]);
        if (hipStreamSynchronize(cv.streams[k]) != hipSuccess && rc == G16_OK) rc = G16_ERR_HIP;
        bufs[k].release();
    }
    return rc;
}

constexpr int WINDOWS = 64, DIGITS = 15;   // 4-bit windows of a 256-bit scalar; table entry [base][window][digit - 1]

template <class C>
using Aff1 = Affine<typename Pairing<C>::F>;

// per-device part of a prepared key
template <class C>
struct PvkDev {
    typedef Pairing<C> PP;
    int device = -1;
    typename PP::Ell* lines = nullptr;   // [2][NCOEFF]: -gamma, -delta
    Aff1<C>* tables = nullptr;           // [nb][WINDOWS][DIGITS]
    typename PP::F12* ab = nullptr;      // e(alpha, beta)
    typename C::G1A* gabc0 = nullptr;    // gamma_abc_g1[0]
    int id_flags = 0;                    // bit 0: gamma is the identity, bit 1: delta is (their pairs contribute 1)
    void release() {
        if (device >= 0) (void)hipSetDevice(device);
        (void)hipFree(lines);
        (void)hipFree(tables);
        (void)hipFree(ab);
        (void)hipFree(gabc0);
        lines = nullptr; tables = nullptr; ab = nullptr; gabc0 = nullptr;
    }
};

// one table entry: d * 2^(4w) * b for 0 <= w < WINDOWS, 1 <= d <= DIGITS (the identity for the identity).  The text of
// verify_window_table_kernel and of the host builder behind g16_host_pvk_tables / g16_host_prepare_inputs (preplab.hip).
template <class C>
G16_HD Aff1<C> window_table_entry(const typename C::G1A& b, int w, int d) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    if (b.is_identity()) return Aff1<C>::identity();
    const typename PP::A1 p = PP::g1_in(b);
    uint32_t k[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    k[w >> 3] = (uint32_t)d << (4 * (w & 7));
    const XYZZ<F> r = XYZZ<F>::from_affine(Aff1<C>{p.x, p.y}).mul_bits(k, 4 * w + 4);
    return r.to_affine();
}

// acc += x gamma_abc[j + 1] from a key's window tables; x in Montgomery form
template <class C>
G16_HD void tab_accumulate(XYZZ<typename Pairing<C>::F>& acc, const Aff1<C>* tables, uint64_t j, const typename C::Fr& x) {
    uint32_t k[8];
    x.to_canonical(k);
    for (int w = 0; w < WINDOWS; ++w) {
        const uint32_t d = (k[w >> 3] >> (4 * (w & 7))) & 0xfu;
        if (d) acc.add_affine(tables[(j * WINDOWS + (uint64_t)w) * DIGITS + d - 1]);
    }
}

// IC = gabc0 + sum_j x_j gamma_abc[j + 1] from the window tables; x: num_public Fr (Montgomery)
template <class C>
__device__ __host__ inline Aff1<C> prepare_inputs_tab(const typename C::G1A& gabc0, const Aff1<C>* tables, const typename C::Fr* x,
                                                      uint64_t num_public) {
    typedef typename Pairing<C>::F F;
    XYZZ<F> acc = XYZZ<F>::identity();
    if (!gabc0.is_identity()) {
        const typename Pairing<C>::A1 g = Pairing<C>::g1_in(gabc0);
        acc = XYZZ<F>::from_affine(Aff1<C>{g.x, g.y});
    }
    for (uint64_t j = 0; j < num_public; ++j) tab_accumulate<C>(acc, tables, j, x[j]);
    return acc.to_affine();
}

// f *= the loop value (before finish_loop) of p against one row of prepared lines; f enters as the value the loop starts from
template <class C>
G16_HD void miller_prepared(typename Pairing<C>::F12& f, const typename Pairing<C>::Ell* lines, const typename Pairing<C>::A1& p) {
    typedef Pairing<C> PP;
    int idx = 0;
    PP::drive([&](int) { PP::ell(f, lines[idx], p); ++idx; }, [&](bool first) { if (!first) f = f.sqr(); });
}

// e = FE(prod_k ML(g1s[k], g2s[k])) on the host; false: the loop gave 0
template <class C>
bool host_pairing_product(const uint64_t* g1s, const uint64_t* g2s, uint64_t n, typename Pairing<C>::F12& e) {
    typedef Pairing<C> PP;
    typename PP::F12 f = PP::F12::one();
    for (uint64_t k = 0; k < n; ++k) {
        typename PP::LiveQ lq;
        typename PP::A1 pa;
        bool skip;
        const typename C::G1A p = ld<typename C::G1A>(g1s + k * C::Fq::N);
        const typename C::G2A q = ld<typename C::G2A>(g2s + k * 2 * C::Fq::N);
        f = f * PP::miller_live(&p, &q, 1, &lq, &pa, &skip);
    }
    return PP::final_exp(f, e);
}

// e(alpha, beta) of a key on the host
template <class C>
int host_alpha_beta(const g16_vk_view* vk, typename Pairing<C>::F12& ab) {
    return host_pairing_product<C>(vk->alpha_g1, vk->beta_g2, 1, ab) ? G16_OK : G16_ERR_UNEXPECTED_IDENTITY;
}

// ---- shared by the aggregate forms (verify_aggregate.hip: one key per call, verify_mixed.hip: keys mixed in one call) ----------
constexpr int AGG_MAX_PER_LANE = 4;   // proofs that may share a lane's accumulator

// the caller's coefficients (none may be zero) or fresh ones from the operating system's generator (verify_aggregate.hip)
int agg_coeffs(const uint64_t* coeffs, uint64_t n, std::vector<uint64_t>& own, const uint64_t** out);

// a 128-bit coefficient (two words of caller memory) as 32-bit words, and in Fr
G16_HD void coeff_words(const uint64_t* c, uint32_t* k) {
    k[0] = (uint32_t)c[0]; k[1] = (uint32_t)(c[0] >> 32); k[2] = (uint32_t)c[1]; k[3] = (uint32_t)(c[1] >> 32);
}
template <class Fr>
G16_HD Fr coeff_fr(const uint64_t* c) {
    uint32_t k[Fr::N] = {};
    coeff_words(c, k);
    return Fr::from_canonical(k);
}

// The per-proof stage for cnt <= AGG_MAX_PER_LANE proofs: f = prod ML'(r_i A_i, B_i) (the loop value before finish_loop),
// sc = sum r_i C_i.  false: a point is off its curve (f and sc are then not used).
template <class C>
G16_HD bool agg_terms(const uint64_t* proofs, const uint64_t* coeffs, int cnt, typename Pairing<C>::F12& f,
                      XYZZ<typename Pairing<C>::F>& sc) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    constexpr int L = C::Fq::N / 2;
    typename PP::LiveQ lq[AGG_MAX_PER_LANE];
    typename PP::A1 pa[AGG_MAX_PER_LANE];
    bool live[AGG_MAX_PER_LANE];
    bool on_curve = true, any = false;
    f = PP::F12::one();
    sc = XYZZ<F>::identity();
    for (int k = 0; k < cnt; ++k) {
        const uint64_t* pr = proofs + (size_t)k * 8 * L;
        const typename C::G1A A = ld_any<typename C::G1A>(pr);
        const typename C::G2A B = ld_any<typename C::G2A>(pr + 2 * L);
        const typename C::G1A Cc = ld_any<typename C::G1A>(pr + 6 * L);
        live[k] = false;
        if (!PP::g1_on_curve(A) || !PP::g2_on_curve(B) || !PP::g1_on_curve(Cc)) { on_curve = false; continue; }
        uint32_t r[4];
        coeff_words(coeffs + 2 * k, r);
        if (!A.is_identity() && !B.is_identity()) {
            const typename PP::A1 a = PP::g1_in(A);
            const Aff1<C> ra = XYZZ<F>::from_affine(Aff1<C>{a.x, a.y}).mul_bits(r, 128).to_affine();
            if (!ra.is_identity()) {   // r_i A_i = 0 only for an A outside the prime-order subgroup
                live[k] = any = true;
                pa[k] = {ra.x, ra.y};
                lq[k].init(PP::g2_in(B));
            }
        }
        if (!Cc.is_identity()) {
            const typename PP::A1 c = PP::g1_in(Cc);
            sc.add(XYZZ<F>::from_affine(Aff1<C>{c.x, c.y}).mul_bits(r, 128));
        }
    }
    if (!on_curve) return false;
    if (any)
        PP::drive([&](int step) {
                      for (int k = 0; k < cnt; ++k)
                          if (live[k]) { const typename PP::Ell e = lq[k].next(step); PP::ell(f, e, pa[k]); }
                  },
                  [&](bool first) { if (!first) f = f.sqr(); });
    return true;
}

template <class T>
__device__ inline T wave_shfl_down(const T& v, int d) {
    static_assert(sizeof(T) % 4 == 0, "moved as 32-bit words");
    T r;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
    uint32_t* t = reinterpret_cast<uint32_t*>(&r);
    // kept a loop over the words in scratch: unrolled, a whole Fq12 would sit in registers on either side of the move
#pragma nounroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k) t[k] = (uint32_t)__shfl_down((int)s[k], d, 64);
    return r;
}

// lane 0 ends with the product of the wave's f and the sum of its sc (the other lanes' values are not meaningful).  One interleaved
// loop, not wave_product followed by wave_sum: that is the text the miller and reduce kernels' resource figures belong to.
template <class C>
__device__ inline void wave_reduce(typename Pairing<C>::F12& f, XYZZ<typename Pairing<C>::F>& sc) {
    for (int d = 32; d >= 1; d >>= 1) {
        const typename Pairing<C>::F12 g = wave_shfl_down(f, d);
        const XYZZ<typename Pairing<C>::F> h = wave_shfl_down(sc, d);
        f = f * g;
        sc.add(h);
    }
}

// lane 0 ends with the product of the wave's values
template <class C>
__device__ inline void wave_product(typename Pairing<C>::F12& f) {
    for (int d = 32; d >= 1; d >>= 1) {
        const typename Pairing<C>::F12 g = wave_shfl_down(f, d);
        f = f * g;
    }
}

// lane 0 ends with the sum of the wave's points
template <class C>
__device__ inline void wave_sum(XYZZ<typename Pairing<C>::F>& sc) {
    for (int d = 32; d >= 1; d >>= 1) {
        const XYZZ<typename Pairing<C>::F> h = wave_shfl_down(sc, d);
        sc.add(h);
    }
}

template <class Fr>
__device__ inline Fr agg_block_sum(Fr acc, Fr* sh) {
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned d = blockDim.x / 2; d >= 1; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + d];
        __syncthreads();
    }
    return sh[0];
}

// The membership stage inside an aggregate call: the tests of verify_subgroup.hip over the n proofs at d_proofs, the copy the Miller
// stage is about to read, on the same stream.  *summary (host) holds subgroup_enqueue_proofs' summary word once s has been waited for.
inline int agg_membership_enqueue(hipStream_t s, int curve, const uint64_t* d_proofs, uint64_t n, DevBufs& bufs, int* summary) {
    uint8_t *d_pt, *d_flags;
    int* d_sub;
    G16_TRY(bufs.get(&d_pt, 3 * n));
    G16_TRY(bufs.get(&d_flags, n));
    G16_TRY(bufs.get(&d_sub, 1));
    G16_HIP_TRY(hipMemsetAsync(d_sub, 0, sizeof(int), s));
    G16_TRY(subgroup_enqueue_proofs(s, curve, d_proofs, n, d_pt, d_flags, d_sub));
    G16_HIP_TRY(hipMemcpyAsync(summary, d_sub, sizeof(int), hipMemcpyDeviceToHost, s));
    return G16_OK;
}

// the verdict that the stages before the equation already decide, in their precedence: 4 some proof's bytes do not decode, 2 a point
// is off its curve, 3 a point is outside its subgroup; 0: the equation decides.  off_subgroup: the membership stage's summary word
inline uint8_t agg_early_verdict(int undecodable, int off_curve, int off_subgroup) {
    if (undecodable) return 4;
    if (off_curve || (off_subgroup & 2)) return 2;
    return off_subgroup ? 3 : 0;
}

// ---- the once-per-batch tail of the aggregate equation (host) ------------------------------------------------------------------
// One key's side of it: g = ML(S_IC, -gamma) ML(sc, -delta) (finished loops) and rhs = ab^s, for sc = the key's sum of r_i C_i,
// st = (s, t_1 .. t_(n_gamma_abc - 1)) and ab = e(alpha, beta).  S_IC by variable-base multiplication: once per call.
template <class C>
void agg_key_tail(const XYZZ<typename Pairing<C>::F>& sc, const typename C::Fr* st, uint64_t n_gamma_abc, const uint64_t* gamma_g2,
                  const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, const typename Pairing<C>::F12& ab, typename Pairing<C>::F12& g,
                  typename Pairing<C>::F12& rhs) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    constexpr int L = C::Fq::N / 2;
    XYZZ<F> sic = XYZZ<F>::identity();
    for (uint64_t j = 0; j < n_gamma_abc; ++j) {
        const G1A gj = ld<G1A>(gamma_abc_g1 + j * 2 * L);
        if (gj.is_identity()) continue;
        const typename PP::A1 p = PP::g1_in(gj);
        uint32_t k[8];
        st[j].to_canonical(k);
        sic.add(XYZZ<F>::from_affine(Aff1<C>{p.x, p.y}).mul_bits(k, 256));
    }
    const Aff1<C> pts[2] = {sic.to_affine(), sc.to_affine()};
    G1A ps[2] = {G1A::identity(), G1A::identity()};
    for (int k = 0; k < 2; ++k)
        if (!pts[k].is_identity()) { ps[k].x = pts[k].x.to_std(); ps[k].y = pts[k].y.to_std(); }
    G2A qs[2] = {ld<G2A>(gamma_g2).neg(), ld<G2A>(delta_g2).neg()};
    typename PP::LiveQ lq[2];
    typename PP::A1 pa[2];
    bool skip[2];
    g = PP::miller_live(ps, qs, 2, lq, pa, skip);
    uint32_t s[8];
    st[0].to_canonical(s);
    rhs = PP::cyc_pow_bits(ab, s, 256);
}

// The closing step: lhs = FE(finish_loop(f) g) for f = the product of the per-proof loop values (before finish_loop) and g = the
// product of the keys' finished loops, against rhs.  lhs / rhs (ark form) are written when given, verdict (1 / 0) when given.  A loop
// value of 0 is verdict 0, or an error for a caller that asked for lhs.
template <class C>
int agg_finish(const typename Pairing<C>::F12& f, const typename Pairing<C>::F12& g, const typename Pairing<C>::F12& rhs, uint8_t* verdict,
               uint64_t* lhs_out, uint64_t* rhs_out) {
    typedef Pairing<C> PP;
    typename PP::F12 lhs;
    if (!PP::final_exp(PP::finish_loop(f) * g, lhs)) {
        if (lhs_out) return G16_ERR_UNEXPECTED_IDENTITY;
        *verdict = 0;
        return G16_OK;
    }
    if (lhs_out) PP::store_gt(lhs, lhs_out);
    if (rhs_out) PP::store_gt(rhs, rhs_out);
    if (verdict) *verdict = PP::equal(lhs, rhs) ? 1 : 0;
    return G16_OK;
}

}  // namespace g16

// one prepared key: the curve, e(alpha, beta) in ark form, and one resident copy per device of the context.  gamma_g2, delta_g2 and
// gamma_abc_g1 are also kept on the host (arkworks form) for the once-per-batch tail of g16_verify_aggregate.
struct g16_pvk {
    int curve = 0;
    uint64_t n_gamma_abc = 0;
    uint64_t ab[72] = {};
    std::vector<uint64_t> gamma_g2, delta_g2, gamma_abc_g1;
    std::vector<g16::PvkDev<g16::Bls12_381>> bls;
    std::vector<g16::PvkDev<g16::Bn254>> bn;
    ~g16_pvk() {
        for (auto& d : bls) d.release();
        for (auto& d : bn) d.release();
    }
};

namespace g16 {
template <class C>
inline std::vector<PvkDev<C>>& devs_of(g16_pvk* p);
template <>
inline std::vector<PvkDev<Bls12_381>>& devs_of<Bls12_381>(g16_pvk* p) { return p->bls; }
template <>
inline std::vector<PvkDev<Bn254>>& devs_of<Bn254>(g16_pvk* p) { return p->bn; }

inline bool vk_view_ok(const g16_vk_view* vk) {
    return vk && vk->alpha_g1 && vk->beta_g2 && vk->gamma_g2 && vk->delta_g2 && vk->gamma_abc_g1 && vk->n_gamma_abc >= 1;
}
}  // namespace g16

#define G16_VERIFY_DISPATCH(curve, EXPR)                                                  \
    do {                                                                                  \
        try {                                                                             \
            if ((curve) == G16_BLS12_381) { typedef Bls12_381 CC; return EXPR; }          \
            if ((curve) == G16_BN254) { typedef Bn254 CC; return EXPR; }                  \
            return G16_ERR_BAD_ARG;                                                       \
        } catch (const std::bad_alloc&) {                                                 \
            return G16_ERR_OOM;                                                           \
        } catch (...) {                                                                   \
            return G16_ERR_INTERNAL;                                                      \
        }                                                                                 \
    } while (0)
