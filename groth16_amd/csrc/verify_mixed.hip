// Randomised batch verification of Groth16 proofs made under SEVERAL verifying keys: still one equation and one final
// exponentiation per call.  With key_of[i] = k naming the key of proof i,
//
//     FE( prod_i ML(r_i A_i, B_i) * prod_k [ ML(S_IC_k, -gamma_k) * ML(S_C_k, -delta_k) ] ) == prod_k e(alpha_k, beta_k)^(s_k)
//     s_k = sum_{i in k} r_i,  t_kj = sum_{i in k} r_i x_ij,  S_IC_k = s_k gamma_abc_k[0] + sum_j t_kj gamma_abc_k[j + 1],
//     S_C_k = sum_{i in k} r_i C_i.
//
// The live pair per proof does not depend on the key and is the per-proof function of the single-key form (agg_terms,
// verify_common.hpp); what is per key runs on the GPU too, one lane per key, because K host tails do not scale.  ONE path for every K:
//
//   host                        counting sort of the proofs by key (the proofs themselves stay in the caller's order, the kernels
//                               read them through `order`), per-key ranges, per-proof offsets into the ragged public inputs, the
//                               flat (key, column) list of the scalar stage, one descriptor per key that has proofs.
//   verify_mixed_scalar_kernel  one workgroup per (key, column): s_k and the t_kj over the key's range.
//   verify_mixed_key_kernel     one lane per key, on a second stream beside the per-proof stage (it needs the Fr sums only): S_IC_k
//                               from the key's window tables, its Miller loop on the prepared lines of -gamma_k, and
//                               e(alpha_k, beta_k)^(s_k) as a cyclotomic power.  The wave multiplies its lanes' values.
//   verify_mixed_miller_kernel  one proof per lane in grouped order (no lane sharing: a lane's sum of r_i C_i must not mix keys).
//                               The wave multiplies its f into one value (the product is global) and adds its r_i C_i PER RUN OF
//                               EQUAL KEYS; the head of each run writes one record.  A key's records are contiguous.
//   verify_mixed_csum_kernel    one wave per key: S_C_k = the sum of the key's records.
//   verify_mixed_delta_kernel   one lane per key: the Miller loop of S_C_k on the prepared lines of -delta_k.
//   verify_mixed_reduce_kernel  products of 64 Fq12 values at a time, until at most 64 are left for the host.
//   host                        finish_loop(product of every loop value), ONE final exponentiation, the comparison with the product
//                               of the GT powers.  Verdict rules as g16_verify_aggregate.
// A multi-device context runs the call on its first device.  g16_host_verify_aggregate_mixed runs the same templates on the CPU.
#include "verify_common.hpp"

using namespace g16;

namespace g16 {

constexpr int MIXED_SCALAR_BLOCK = 256;
constexpr uint32_t MIXED_NO_KEY = 0xffffffffu;   // the key of a lane past the batch

// a key that has proofs in this call: pointers into its PvkDev and its place in the call's arrays
template <class C>
struct MixedKeyDev {
    const typename Pairing<C>::Ell* lines;
    const Aff1<C>* tables;
    const typename Pairing<C>::F12* ab;
    const typename C::G1A* gabc0;
    int id_flags;
    uint32_t num_public;
    uint64_t lo, hi;    // its proofs in grouped order
    uint64_t st_off;    // its num_public + 1 Fr sums (s, t_1 ..)
    uint64_t rec_off;   // its records of partial sums of r_i C_i: one per wave its range touches
};

G16_HD uint64_t mixed_records(uint64_t lo, uint64_t hi) { return (hi - 1) / VERIFY_BLOCK - lo / VERIFY_BLOCK + 1; }

struct MixedCol { uint32_t key, col; };

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// workgroup b: column cols[b].col of key cols[b].key -- 0 sums the r_i of the key's proofs, j > 0 the r_i x_i(j-1)
template <class C>
__global__ __launch_bounds__(MIXED_SCALAR_BLOCK) void verify_mixed_scalar_kernel(const MixedKeyDev<C>* keys, const MixedCol* cols,
                                                                                const uint32_t* order, const uint64_t* x_off,
                                                                                const uint64_t* coeffs, const uint64_t* inputs,
                                                                                typename C::Fr* st) {
    typedef typename C::Fr Fr;
    __shared__ Fr sh[MIXED_SCALAR_BLOCK];
    const MixedCol kc = cols[blockIdx.x];
    const uint64_t lo = keys[kc.key].lo, hi = keys[kc.key].hi;
    const uint64_t j = kc.col;
    const Fr* x = reinterpret_cast<const Fr*>(inputs);
    Fr acc = Fr::zero();
    for (uint64_t g = lo + threadIdx.x; g < hi; g += MIXED_SCALAR_BLOCK) {
        const uint64_t i = order[g];
        const Fr r = coeff_fr<Fr>(coeffs + 2 * i);
        acc = acc + (j ? r * x[x_off[i] + (j - 1)] : r);
    }
    const Fr sum = agg_block_sum(acc, sh);
    if (threadIdx.x == 0) st[keys[kc.key].st_off + j] = sum;
}

// lane g: the proof order[g], whose key is gkey[g] (non-decreasing in g).  f_out[workgroup]: the product of the wave's loop values;
// rec: one sum of r_i C_i per run of equal keys in the wave, at the key's rec_off + (this wave - the key's first wave)
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, 2) void verify_mixed_miller_kernel(const uint64_t* proofs, const uint64_t* coeffs,
                                                                            const uint32_t* order, const uint32_t* gkey,
                                                                            const MixedKeyDev<C>* keys, uint64_t n,
                                                                            typename Pairing<C>::F12* f_out,
                                                                            XYZZ<typename Pairing<C>::F>* rec, int* off_curve) {
    typedef Pairing<C> PP;
    typedef XYZZ<typename PP::F> G1X;
    constexpr int L = C::Fq::N / 2;
    const uint64_t g = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    const uint32_t key = g < n ? gkey[g] : MIXED_NO_KEY;
    typename PP::F12 f = PP::F12::one();
    G1X sc = G1X::identity();
    if (g < n) {
        const uint64_t i = order[g];
        if (!agg_terms<C>(proofs + i * 8 * L, coeffs + i * 2, 1, f, sc)) {
            atomicOr(off_curve, 1);
            f = PP::F12::one();
            sc = G1X::identity();
        }
    }
    // After the step with distance d a lane holds the product of the f of lanes [l, l + 2d) and the sum of the sc of those among
    // them that lie in its own run of equal keys (the keys are sorted, so a run is an interval of lanes).  Lanes whose interval
    // leaves the wave hold values that no lane of a full interval reads.
    for (int d = 1; d < VERIFY_BLOCK; d <<= 1) {
        const typename PP::F12 fd = wave_shfl_down(f, d);
        const G1X hd = wave_shfl_down(sc, d);
        const uint32_t kd = (uint32_t)__shfl_down((int)key, d, VERIFY_BLOCK);
        f = f * fd;
        if ((int)threadIdx.x + d < VERIFY_BLOCK && kd == key) sc.add(hd);
    }
    const uint32_t before = (uint32_t)__shfl_up((int)key, 1, VERIFY_BLOCK);
    if (key != MIXED_NO_KEY && (threadIdx.x == 0 || before != key))
        rec[keys[key].rec_off + (g / VERIFY_BLOCK - keys[key].lo / VERIFY_BLOCK)] = sc;
    if (threadIdx.x == 0) f_out[blockIdx.x] = f;
}

// workgroup (one wave) a: sc_out[a] = the sum of key a's records
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK) void verify_mixed_csum_kernel(const MixedKeyDev<C>* keys, const XYZZ<typename Pairing<C>::F>* rec,
                                                                         XYZZ<typename Pairing<C>::F>* sc_out) {
    typedef XYZZ<typename Pairing<C>::F> G1X;
    const uint64_t lo = keys[blockIdx.x].lo, hi = keys[blockIdx.x].hi, off = keys[blockIdx.x].rec_off;
    const uint64_t m = mixed_records(lo, hi);
    G1X acc = G1X::identity();
    for (uint64_t r = threadIdx.x; r < m; r += VERIFY_BLOCK) acc.add(rec[off + r]);
    wave_sum<C>(acc);
    if (threadIdx.x == 0) sc_out[blockIdx.x] = acc;
}

// lane a: S_IC of key a from its Fr sums, the loop value of (S_IC, -gamma) before finish_loop, and e(alpha, beta)^s;
// g_out / rhs_out[workgroup]: the products over the wave
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, 2) void verify_mixed_key_kernel(const MixedKeyDev<C>* keys, uint64_t n_active,
                                                                         const typename C::Fr* st, typename Pairing<C>::F12* g_out,
                                                                         typename Pairing<C>::F12* rhs_out) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    const uint64_t a = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    typename PP::F12 f = PP::F12::one(), rhs = PP::F12::one();
    if (a < n_active) {
        const typename C::Fr* t = st + keys[a].st_off;
        const Aff1<C>* tables = keys[a].tables;
        const uint64_t num_public = keys[a].num_public;
        uint32_t s[8];
        t[0].to_canonical(s);
        XYZZ<F> acc = XYZZ<F>::identity();
        const typename C::G1A g0 = *keys[a].gabc0;
        if (!g0.is_identity()) {
            const typename PP::A1 p = PP::g1_in(g0);
            acc = XYZZ<F>::from_affine(Aff1<C>{p.x, p.y}).mul_bits(s, 256);
        }
        for (uint64_t j = 0; j < num_public; ++j) tab_accumulate<C>(acc, tables, j, t[j + 1]);
        const Aff1<C> ic = acc.to_affine();
        if (!ic.is_identity() && !(keys[a].id_flags & 1)) miller_prepared<C>(f, keys[a].lines, {ic.x, ic.y});
        rhs = PP::cyc_pow_bits(*keys[a].ab, s, 256);
    }
    wave_product<C>(f);
    wave_product<C>(rhs);
    if (threadIdx.x == 0) {
        g_out[blockIdx.x] = f;
        rhs_out[blockIdx.x] = rhs;
    }
}

// lane a: the loop value of (S_C of key a, -delta) before finish_loop; f_out[workgroup]: the product over the wave
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, 2) void verify_mixed_delta_kernel(const MixedKeyDev<C>* keys, uint64_t n_active,
                                                                           const XYZZ<typename Pairing<C>::F>* sc,
                                                                           typename Pairing<C>::F12* f_out) {
    typedef Pairing<C> PP;
    const uint64_t a = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    typename PP::F12 f = PP::F12::one();
    if (a < n_active) {
        const Aff1<C> c = sc[a].to_affine();
        if (!c.is_identity() && !(keys[a].id_flags & 2)) miller_prepared<C>(f, keys[a].lines + PP::NCOEFF, {c.x, c.y});
    }
    wave_product<C>(f);
    if (threadIdx.x == 0) f_out[blockIdx.x] = f;
}

// m values in, ceil(m / 64) products out
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK, 2) void verify_mixed_reduce_kernel(const typename Pairing<C>::F12* in, uint64_t m,
                                                                            typename Pairing<C>::F12* out) {
    const uint64_t i = (uint64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    typename Pairing<C>::F12 f = Pairing<C>::F12::one();
    if (i < m) f = in[i];
    wave_product<C>(f);
    if (threadIdx.x == 0) out[blockIdx.x] = f;
}

// ---- the layout of a call (host, O(n)) ----------------------------------------------------------------------------------------
struct MixedLayout {
    std::vector<uint64_t> lo;       // n_keys + 1: key k's proofs are order[lo[k] .. lo[k + 1])
    std::vector<uint32_t> order;    // grouped position -> proof index (stable: input order within a key)
    std::vector<uint64_t> x_off;    // proof index -> first Fr of its public inputs
};

// num_public[k]: the inputs a proof of key k brings
int mixed_layout(const std::vector<uint64_t>& num_public, const uint32_t* key_of, uint64_t n, uint64_t n_public_total, MixedLayout& out) {
    const uint64_t n_keys = num_public.size();
    if (n >> 32) return G16_ERR_BAD_ARG;
    out.lo.assign(n_keys + 1, 0);
    out.x_off.resize(n);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (key_of[i] >= n_keys) return G16_ERR_BAD_ARG;
        ++out.lo[key_of[i] + 1];
        out.x_off[i] = total;
        total += num_public[key_of[i]];
    }
    if (total != n_public_total) return G16_ERR_MALFORMED_VK;
    for (uint64_t k = 0; k < n_keys; ++k) out.lo[k + 1] += out.lo[k];
    std::vector<uint64_t> next(out.lo.begin(), out.lo.end() - 1);
    out.order.resize(n);
    for (uint64_t i = 0; i < n; ++i) out.order[next[key_of[i]]++] = (uint32_t)i;
    return G16_OK;
}

// ---- host form ------------------------------------------------------------------------------------------------------------------
template <class C>
int host_verify_mixed(const g16_vk_view* vks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs, uint64_t n,
                      const uint64_t* inputs, uint64_t n_public_total, const uint64_t* coeffs, uint8_t* verdict, uint64_t* lhs_out,
                      uint64_t* rhs_out) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    typedef typename C::Fr Fr;
    constexpr int L = C::Fq::N / 2;
    std::vector<uint64_t> num_public(n_keys);
    for (uint64_t k = 0; k < n_keys; ++k) num_public[k] = vks[k].n_gamma_abc - 1;
    MixedLayout lay;
    G16_TRY(mixed_layout(num_public, key_of, n, n_public_total, lay));
    if (!n) { *verdict = 1; return G16_OK; }
    std::vector<uint64_t> own;
    const uint64_t* r = nullptr;
    G16_TRY(agg_coeffs(coeffs, n, own, &r));
    typename PP::F12 f = PP::F12::one(), g = PP::F12::one(), rhs = PP::F12::one();
    bool on_curve = true;
    for (uint64_t k = 0; k < n_keys; ++k) {
        const uint64_t lo = lay.lo[k], hi = lay.lo[k + 1];
        if (lo == hi) continue;
        XYZZ<F> sc = XYZZ<F>::identity();
        std::vector<Fr> st(num_public[k] + 1, Fr::zero());
        for (uint64_t p = lo; p < hi; p += AGG_MAX_PER_LANE) {   // in groups that share an accumulator, as g16_host_verify_aggregate
            const int cnt = (int)std::min<uint64_t>(AGG_MAX_PER_LANE, hi - p);
            uint64_t pbuf[AGG_MAX_PER_LANE * 8 * L], rbuf[AGG_MAX_PER_LANE * 2];
            for (int c = 0; c < cnt; ++c) {
                const uint64_t i = lay.order[p + c];
                memcpy(pbuf + (size_t)c * 8 * L, proofs + i * 8 * L, 8 * L * sizeof(uint64_t));
                rbuf[2 * c] = r[2 * i];
                rbuf[2 * c + 1] = r[2 * i + 1];
                const Fr ri = coeff_fr<Fr>(r + 2 * i);
                st[0] = st[0] + ri;
                for (uint64_t j = 0; j < num_public[k]; ++j) st[j + 1] = st[j + 1] + ri * ld<Fr>(inputs + (lay.x_off[i] + j) * 4);
            }
            typename PP::F12 fi;
            XYZZ<F> ci;
            if (!agg_terms<C>(pbuf, rbuf, cnt, fi, ci)) { on_curve = false; continue; }
            f = f * fi;
            sc.add(ci);
        }
        if (!on_curve) continue;
        typename PP::F12 ab, gk, rk;
        G16_TRY(host_alpha_beta<C>(&vks[k], ab));
        agg_key_tail<C>(sc, st.data(), vks[k].n_gamma_abc, vks[k].gamma_g2, vks[k].delta_g2, vks[k].gamma_abc_g1, ab, gk, rk);
        g = g * gk;
        rhs = rhs * rk;
    }
    if (!on_curve) {
        if (lhs_out) return G16_ERR_BAD_ARG;
        *verdict = 2;
        return G16_OK;
    }
    return agg_finish<C>(f, g, rhs, verdict, lhs_out, rhs_out);
}

// ---- device side of g16_verify_aggregate_mixed ---------------------------------------------------------------------------------
template <class C>
int mixed_any(g16_ctx* ctx, const g16_pvk* const* pvks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs, uint64_t n,
              const uint64_t* inputs, uint64_t n_public_total, const uint64_t* coeffs, bool check, uint8_t* verdict) {
    typedef Pairing<C> PP;
    typedef typename PP::F12 F12;
    typedef XYZZ<typename PP::F> G1X;
    typedef typename C::Fr Fr;
    constexpr int L = C::Fq::N / 2;
    CtxView cv;
    G16_TRY(cv.load(ctx));
    std::vector<uint64_t> num_public(n_keys);
    for (uint64_t k = 0; k < n_keys; ++k) {
        if (!pvks[k] || pvks[k]->curve != cv.curve) return G16_ERR_BAD_ARG;
        const std::vector<PvkDev<C>>& pd = devs_of<C>(const_cast<g16_pvk*>(pvks[k]));
        if (pd.size() != cv.devs.size() || pd[0].device != cv.devs[0]) return G16_ERR_BAD_ARG;   // the key was loaded on another context
        num_public[k] = pvks[k]->n_gamma_abc - 1;
    }
    MixedLayout lay;
    G16_TRY(mixed_layout(num_public, key_of, n, n_public_total, lay));
    if (!n) { *verdict = 1; return G16_OK; }
    std::vector<uint64_t> own;
    const uint64_t* r = nullptr;
    G16_TRY(agg_coeffs(coeffs, n, own, &r));

    // the keys that have proofs, their places in the call's arrays, the key of every grouped position, the scalar stage's columns
    std::vector<MixedKeyDev<C>> keys;
    std::vector<uint32_t> gkey(n);
    std::vector<MixedCol> cols;
    uint64_t n_st = 0, n_rec = 0;
    for (uint64_t k = 0; k < n_keys; ++k) {
        const uint64_t lo = lay.lo[k], hi = lay.lo[k + 1];
        if (lo == hi) continue;
        const PvkDev<C>& d = devs_of<C>(const_cast<g16_pvk*>(pvks[k]))[0];
        const uint32_t a = (uint32_t)keys.size();
        keys.push_back({d.lines, d.tables, d.ab, d.gabc0, d.id_flags, (uint32_t)num_public[k], lo, hi, n_st, n_rec});
        n_st += num_public[k] + 1;
        n_rec += mixed_records(lo, hi);
        for (uint64_t p = lo; p < hi; ++p) gkey[p] = a;
        for (uint64_t j = 0; j <= num_public[k]; ++j) cols.push_back({a, (uint32_t)j});
    }
    const uint64_t n_active = keys.size();
    const uint64_t blocks = (n + VERIFY_BLOCK - 1) / VERIFY_BLOCK, kw = (n_active + VERIFY_BLOCK - 1) / VERIFY_BLOCK;
    const uint64_t n_f = blocks + 2 * kw;   // the loop values: per workgroup of the per-proof stage, of the delta stage, of the key stage

    const int device = cv.devs[0];
    hipStream_t s = cv.streams[0], side = nullptr;
    hipEvent_t ev_st = nullptr, ev_key = nullptr;
    DevBufs bufs;
    std::vector<F12> h_f, h_rhs;
    int off_curve = 0, off_subgroup = 0;
    int rc = [&]() -> int {
        G16_HIP_TRY(hipSetDevice(device));
        G16_HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        G16_HIP_TRY(hipEventCreateWithFlags(&ev_st, hipEventDisableTiming));
        G16_HIP_TRY(hipEventCreateWithFlags(&ev_key, hipEventDisableTiming));
        uint64_t *d_proofs, *d_coeffs, *d_inputs, *d_xoff;
        uint32_t *d_order, *d_gkey;
        MixedKeyDev<C>* d_keys;
        MixedCol* d_cols;
        Fr* d_st;
        G1X *d_rec, *d_sc;
        F12 *d_f[2], *d_rhs[2];
        int* d_off;
        G16_TRY(bufs.get(&d_proofs, n * 8 * L));
        G16_TRY(bufs.get(&d_coeffs, n * 2));
        G16_TRY(bufs.get(&d_inputs, n_public_total * 4));
        G16_TRY(bufs.get(&d_xoff, n));
        G16_TRY(bufs.get(&d_order, n));
        G16_TRY(bufs.get(&d_gkey, n));
        G16_TRY(bufs.get(&d_keys, n_active));
        G16_TRY(bufs.get(&d_cols, cols.size()));
        G16_TRY(bufs.get(&d_st, n_st));
        G16_TRY(bufs.get(&d_rec, n_rec));
        G16_TRY(bufs.get(&d_sc, n_active));
        G16_TRY(bufs.get(&d_f[0], n_f));
        G16_TRY(bufs.get(&d_f[1], (n_f + VERIFY_BLOCK - 1) / VERIFY_BLOCK));
        G16_TRY(bufs.get(&d_rhs[0], kw));
        G16_TRY(bufs.get(&d_rhs[1], (kw + VERIFY_BLOCK - 1) / VERIFY_BLOCK));
        G16_TRY(bufs.get(&d_off, 1));
        G16_HIP_TRY(hipMemcpyAsync(d_coeffs, r, n * 2 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        if (n_public_total) G16_HIP_TRY(hipMemcpyAsync(d_inputs, inputs, n_public_total * 4 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        G16_HIP_TRY(hipMemcpyAsync(d_xoff, lay.x_off.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        G16_HIP_TRY(hipMemcpyAsync(d_order, lay.order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        G16_HIP_TRY(hipMemcpyAsync(d_gkey, gkey.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        G16_HIP_TRY(hipMemcpyAsync(d_keys, keys.data(), n_active * sizeof(MixedKeyDev<C>), hipMemcpyHostToDevice, s));
        G16_HIP_TRY(hipMemcpyAsync(d_cols, cols.data(), cols.size() * sizeof(MixedCol), hipMemcpyHostToDevice, s));
        G16_HIP_TRY(hipMemsetAsync(d_off, 0, sizeof(int), s));
        // the Fr sums first: the key stage needs nothing else and runs on the second stream beside everything below
        verify_mixed_scalar_kernel<C><<<(unsigned)cols.size(), MIXED_SCALAR_BLOCK, 0, s>>>(d_keys, d_cols, d_order, d_xoff, d_coeffs, d_inputs, d_st);
        G16_LAUNCH_CHECK();
        G16_HIP_TRY(hipEventRecord(ev_st, s));
        G16_HIP_TRY(hipStreamWaitEvent(side, ev_st, 0));
        verify_mixed_key_kernel<C><<<(unsigned)kw, VERIFY_BLOCK, 0, side>>>(d_keys, n_active, d_st, d_f[0] + blocks + kw, d_rhs[0]);
        G16_LAUNCH_CHECK();
        G16_HIP_TRY(hipEventRecord(ev_key, side));
        G16_HIP_TRY(hipMemcpyAsync(d_proofs, proofs, n * 8 * L * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        if (check) G16_TRY(agg_membership_enqueue(s, C::CURVE_ID, d_proofs, n, bufs, &off_subgroup));
        verify_mixed_miller_kernel<C><<<(unsigned)blocks, VERIFY_BLOCK, 0, s>>>(d_proofs, d_coeffs, d_order, d_gkey, d_keys, n, d_f[0], d_rec, d_off);
        G16_LAUNCH_CHECK();
        verify_mixed_csum_kernel<C><<<(unsigned)n_active, VERIFY_BLOCK, 0, s>>>(d_keys, d_rec, d_sc);
        G16_LAUNCH_CHECK();
        verify_mixed_delta_kernel<C><<<(unsigned)kw, VERIFY_BLOCK, 0, s>>>(d_keys, n_active, d_sc, d_f[0] + blocks);
        G16_LAUNCH_CHECK();
        G16_HIP_TRY(hipStreamWaitEvent(s, ev_key, 0));
        auto reduce = [&](F12** d, uint64_t m, std::vector<F12>& out) -> int {
            int cur = 0;
            for (; m > VERIFY_BLOCK; m = (m + VERIFY_BLOCK - 1) / VERIFY_BLOCK, cur ^= 1) {
                verify_mixed_reduce_kernel<C><<<(unsigned)((m + VERIFY_BLOCK - 1) / VERIFY_BLOCK), VERIFY_BLOCK, 0, s>>>(d[cur], m, d[cur ^ 1]);
                G16_LAUNCH_CHECK();
            }
            out.resize(m);
            G16_HIP_TRY(hipMemcpyAsync(out.data(), d[cur], m * sizeof(F12), hipMemcpyDeviceToHost, s));
            return G16_OK;
        };
        G16_TRY(reduce(d_f, n_f, h_f));
        G16_TRY(reduce(d_rhs, kw, h_rhs));
        G16_HIP_TRY(hipMemcpyAsync(&off_curve, d_off, sizeof(int), hipMemcpyDeviceToHost, s));
        return G16_OK;
    }();
    (void)hipSetDevice(device);
    if (side && hipStreamSynchronize(side) != hipSuccess && rc == G16_OK) rc = G16_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess && rc == G16_OK) rc = G16_ERR_HIP;
    bufs.release();
    if (ev_st) (void)hipEventDestroy(ev_st);
    if (ev_key) (void)hipEventDestroy(ev_key);
    if (side) (void)hipStreamDestroy(side);
    if (rc != G16_OK) return rc;
    if (const uint8_t v = agg_early_verdict(0, off_curve, off_subgroup)) { *verdict = v; return G16_OK; }
    F12 f = F12::one(), rhs = F12::one();
    for (const F12& v : h_f) f = f * v;
    for (const F12& v : h_rhs) rhs = rhs * v;
    F12 lhs;
    *verdict = (PP::final_exp(PP::finish_loop(f), lhs) && PP::equal(lhs, rhs)) ? 1 : 0;
    return G16_OK;
}

static bool mixed_args_ok(const void* keys, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs, uint64_t n,
                          const uint64_t* inputs, uint64_t n_public_total) {
    return (keys || !n_keys) && (n_keys || !n) && (!n || (key_of && proofs)) && (!n_public_total || inputs);
}

}  // namespace g16

extern "C" {

int g16_verify_aggregate_mixed(g16_ctx* ctx, const g16_pvk* const* pvks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs,
                               uint64_t n, const uint64_t* public_inputs, uint64_t n_public_total, const uint64_t* coeffs,
                               int check_subgroups, uint8_t* verdict) {
    if (!ctx || !verdict || !mixed_args_ok(pvks, n_keys, key_of, proofs, n, public_inputs, n_public_total)) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(ctx_curve(ctx), (mixed_any<CC>(ctx, pvks, n_keys, key_of, proofs, n, public_inputs, n_public_total, coeffs,
                                              check_subgroups != 0, verdict)));
}

int g16_host_verify_aggregate_mixed(int curve, const g16_vk_view* vks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs,
                                    uint64_t n, const uint64_t* public_inputs, uint64_t n_public_total, const uint64_t* coeffs,
                                    uint8_t* verdict) {
    if (!verdict || !mixed_args_ok(vks, n_keys, key_of, proofs, n, public_inputs, n_public_total)) return G16_ERR_BAD_ARG;
    for (uint64_t k = 0; k < n_keys; ++k)
        if (!vk_view_ok(&vks[k])) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(curve, (host_verify_mixed<CC>(vks, n_keys, key_of, proofs, n, public_inputs, n_public_total, coeffs, verdict,
                                                      nullptr, nullptr)));
}

int g16_host_verify_aggregate_mixed_gt(int curve, const g16_vk_view* vks, uint64_t n_keys, const uint32_t* key_of, const uint64_t* proofs,
                                       uint64_t n, const uint64_t* public_inputs, uint64_t n_public_total, const uint64_t* coeffs,
                                       uint64_t* lhs_fq12, uint64_t* rhs_fq12) {
    if (!lhs_fq12 || !rhs_fq12 || !coeffs || !n || !mixed_args_ok(vks, n_keys, key_of, proofs, n, public_inputs, n_public_total))
        return G16_ERR_BAD_ARG;
    for (uint64_t k = 0; k < n_keys; ++k)
        if (!vk_view_ok(&vks[k])) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(curve, (host_verify_mixed<CC>(vks, n_keys, key_of, proofs, n, public_inputs, n_public_total, coeffs, nullptr,
                                                      lhs_fq12, rhs_fq12)));
}

}  // extern "C"
