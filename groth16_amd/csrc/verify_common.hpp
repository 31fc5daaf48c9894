// What verify.hip (one verify_proof per lane), verify_aggregate.hip (one equation per batch under one key) and verify_mixed.hip (one
// equation per batch that mixes keys) share: the prepared key, its per-device part, the window-table form of prepare_inputs, the
// per-proof stage and the wave / workgroup reductions of the aggregate forms, and the curve dispatch of the entry points.
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
// verify_aggregate.hip: g16_verify_aggregate_bytes behind its argument checks (n >= 1)
int aggregate_bytes(g16_ctx* ctx, const g16_pvk* pvk, const uint8_t* proof_bytes, uint64_t n, const uint64_t* inputs, uint64_t num_public,
                    const uint64_t* coeffs, uint8_t* verdict);

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

// device buffers of one call, freed together
struct DevBufs {
    std::vector<void*> p;
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
    for (uint64_t j = 0; j < num_public; ++j) {
        uint32_t k[8];
        x[j].to_canonical(k);
        for (int w = 0; w < WINDOWS; ++w) {
            const uint32_t d = (k[w >> 3] >> (4 * (w & 7))) & 0xfu;
            if (d) acc.add_affine(tables[(j * WINDOWS + (uint64_t)w) * DIGITS + d - 1]);
        }
    }
    return acc.to_affine();
}

// ---- shared by the aggregate forms (verify_aggregate.hip: one key per call, verify_mixed.hip: keys mixed in one call) ----------
constexpr int AGG_MAX_PER_LANE = 4;   // proofs that may share a lane's accumulator

// the caller's coefficients (none may be zero) or fresh ones from the operating system's generator (verify_aggregate.hip)
int agg_coeffs(const uint64_t* coeffs, uint64_t n, std::vector<uint64_t>& own, const uint64_t** out);

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
        const uint32_t r[4] = {(uint32_t)coeffs[2 * k], (uint32_t)(coeffs[2 * k] >> 32), (uint32_t)coeffs[2 * k + 1],
                               (uint32_t)(coeffs[2 * k + 1] >> 32)};
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

// lane 0 ends with the product of the wave's f and the sum of its sc (the other lanes' values are not meaningful)
template <class C>
__device__ inline void wave_reduce(typename Pairing<C>::F12& f, XYZZ<typename Pairing<C>::F>& sc) {
    for (int d = 32; d >= 1; d >>= 1) {
        const typename Pairing<C>::F12 g = wave_shfl_down(f, d);
        const XYZZ<typename Pairing<C>::F> h = wave_shfl_down(sc, d);
        f = f * g;
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
