// Groth16 verification on the GPU (/root/reference/src/verifier.rs:13-76, src/lib.rs:84-96) and the pairing entry points.
//
//   g16_pvk_load        prepare_verifying_key: e(alpha, beta), the line coefficients of -gamma and -delta (ark's G2Prepared) and
//                       4-bit fixed-base window tables of gamma_abc_g1[1..] for prepare_inputs, all computed on the GPU and kept
//                       resident (one copy per device of the context).
//   g16_verify_batch    one lane per proof: on-curve checks, IC = gamma_abc[0] + sum x_i gamma_abc[i+1] from the tables, one
//                       Miller loop over (A, B) (lines computed as it goes), (IC, -gamma) and (C, -delta) (lines read from the
//                       prepared tables), the final exponentiation, and the comparison with e(alpha, beta).
// The arithmetic is pairing.hpp on the 30-bit Montgomery products (fp30.hpp); the host entry points run the same templates.
#include "verify_common.hpp"

using namespace g16;

// the kernels live in namespace g16 (not an anonymous one) so that tools/kernel_occupancy.py can name them
namespace g16 {

// ---- kernels ----------------------------------------------------------------------------------------------------------------
template <class C>
__global__ void pairing_prepare_kernel(const typename C::G2A* qs, typename Pairing<C>::Ell* out) {   // lane k: the lines of -qs[k]
    typedef Pairing<C> PP;
    const int k = threadIdx.x;
    if (k >= 2 || qs[k].is_identity()) return;
    const typename PP::A2 q = PP::g2_in(qs[k]);
    PP::prepare(typename PP::A2{q.x, q.y.neg()}, out + (size_t)k * PP::NCOEFF);
}

// one lane: prod_k e(g1s[k], g2s[k]) (ark form out, Fq12 in the internal form out12 if given); status 1 = the loop gave 0
template <class C>
__global__ void pairing_product_kernel(const typename C::G1A* g1s, const typename C::G2A* g2s, uint64_t n, uint64_t* out,
                                       typename Pairing<C>::F12* out12, int* status) {
    typedef Pairing<C> PP;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    typename PP::F12 f = PP::F12::one();
    for (uint64_t k = 0; k < n; ++k) {
        typename PP::LiveQ lq;
        typename PP::A1 pa;
        bool skip;
        f = f * PP::miller_live(g1s + k, g2s + k, 1, &lq, &pa, &skip);
    }
    typename PP::F12 e;
    *status = PP::final_exp(f, e) ? 0 : 1;
    if (*status) return;
    PP::store_gt(e, out);
    if (out12) *out12 = e;
}

// lane t < nb * WINDOWS * DIGITS: entry (j, w, d) = d * 2^(4w) * bases[j]
template <class C>
__global__ void verify_window_table_kernel(const typename C::G1A* bases, uint64_t nb, Aff1<C>* tables) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb * WINDOWS * DIGITS) return;
    const uint64_t j = t / (WINDOWS * DIGITS);
    const int w = (int)(t / DIGITS % WINDOWS), d = (int)(t % DIGITS) + 1;
    tables[t] = window_table_entry<C>(bases[j], w, d);
}

// one lane per proof.  prepared: IC per proof given (n G1 affine), else computed from the public inputs
template <class C>
__global__ __launch_bounds__(VERIFY_BLOCK) void verify_batch_kernel(const typename Pairing<C>::Ell* lines, const Aff1<C>* tables,
                                                                     const typename Pairing<C>::F12* ab, const typename C::G1A* gabc0,
                                                                     const uint64_t* proofs, const uint64_t* inputs, uint64_t num_public,
                                                                     const uint64_t* prepared, uint64_t n, int id_flags, uint8_t* verdicts) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int L = C::Fq::N / 2;
    const uint64_t* pr = proofs + i * 8 * L;
    const typename C::G1A A = *reinterpret_cast<const typename C::G1A*>(pr);
    const typename C::G2A B = *reinterpret_cast<const typename C::G2A*>(pr + 2 * L);
    const typename C::G1A Cc = *reinterpret_cast<const typename C::G1A*>(pr + 6 * L);
    if (!PP::g1_on_curve(A) || !PP::g2_on_curve(B) || !PP::g1_on_curve(Cc)) { verdicts[i] = 2; return; }
    typename PP::A1 ic;
    bool ic_id;
    if (prepared) {
        const typename C::G1A p = reinterpret_cast<const typename C::G1A*>(prepared)[i];
        ic_id = p.is_identity();
        ic = ic_id ? typename PP::A1{F::zero(), F::zero()} : PP::g1_in(p);
    } else {
        const Aff1<C> p = prepare_inputs_tab<C>(*gabc0, tables, reinterpret_cast<const typename C::Fr*>(inputs) + i * num_public, num_public);
        ic_id = p.is_identity();
        ic = {p.x, p.y};
    }
    const bool ab_live = !A.is_identity() && !B.is_identity();
    const bool c_live = !Cc.is_identity();
    const typename PP::A1 a = ab_live ? PP::g1_in(A) : typename PP::A1{F::zero(), F::zero()};
    const typename PP::A1 c = c_live ? PP::g1_in(Cc) : typename PP::A1{F::zero(), F::zero()};
    typename PP::LiveQ lq;
    lq.init(ab_live ? PP::g2_in(B) : typename PP::A2{PP::F2::zero(), PP::F2::zero()});
    const typename PP::Ell* gl = lines;
    const typename PP::Ell* dl = lines + PP::NCOEFF;
    const bool g_live = !ic_id && !(id_flags & 1), d_live = c_live && !(id_flags & 2);
    typename PP::F12 f = PP::F12::one();
    int idx = 0;
    PP::drive([&](int step) {
                  if (ab_live) { const typename PP::Ell e = lq.next(step); PP::ell(f, e, a); }
                  if (g_live) PP::ell(f, gl[idx], ic);
                  if (d_live) PP::ell(f, dl[idx], c);
                  ++idx;
              },
              [&](bool first) { if (!first) f = f.sqr(); });
    typename PP::F12 e;
    const bool ok = PP::final_exp(PP::finish_loop(f), e);
    verdicts[i] = (ok && PP::equal(e, *ab)) ? 1 : 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <class T>
int dev_upload(DevBufs& bufs, const T* src, size_t n, T** dst) {
    G16_TRY(bufs.get(dst, n));
    if (n) G16_HIP_TRY(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return G16_OK;
}

template <class C>
int pvk_load_dev(int device, const g16_vk_view* vk, PvkDev<C>* d, uint64_t* ab_out) {
    typedef Pairing<C> PP;
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    d->device = device;
    G16_HIP_TRY(hipSetDevice(device));
    const G1A* gabc = reinterpret_cast<const G1A*>(vk->gamma_abc_g1);
    const uint64_t nb = vk->n_gamma_abc - 1;
    G2A qs[2] = {ld<G2A>(vk->gamma_g2), ld<G2A>(vk->delta_g2)};
    d->id_flags = (qs[0].is_identity() ? 1 : 0) | (qs[1].is_identity() ? 2 : 0);
    G1A alpha = ld<G1A>(vk->alpha_g1);
    G2A beta = ld<G2A>(vk->beta_g2);
    DevBufs tmp;   // the call's temporaries, freed on every way out
    G2A *d_q, *d_beta;
    G1A *d_alpha, *d_bases;
    uint64_t* d_out;
    int* d_status;
    G16_TRY(dev_upload(tmp, qs, 2, &d_q));
    G16_TRY(dev_upload(tmp, &alpha, 1, &d_alpha));
    G16_TRY(dev_upload(tmp, &beta, 1, &d_beta));
    G16_HIP_TRY(hipMalloc((void**)&d->gabc0, sizeof(G1A)));
    G16_HIP_TRY(hipMemcpy(d->gabc0, gabc, sizeof(G1A), hipMemcpyHostToDevice));
    G16_TRY(dev_upload(tmp, gabc + 1, (size_t)nb, &d_bases));
    G16_HIP_TRY(hipMalloc((void**)&d->lines, 2 * PP::NCOEFF * sizeof(typename PP::Ell)));
    G16_HIP_TRY(hipMemset(d->lines, 0, 2 * PP::NCOEFF * sizeof(typename PP::Ell)));
    G16_HIP_TRY(hipMalloc((void**)&d->tables, std::max<uint64_t>(nb, 1) * WINDOWS * DIGITS * sizeof(Aff1<C>)));
    G16_HIP_TRY(hipMalloc((void**)&d->ab, sizeof(typename PP::F12)));
    G16_TRY(tmp.get(&d_out, 12 * (C::Fq::N / 2)));
    G16_TRY(tmp.get(&d_status, 1));
    pairing_prepare_kernel<C><<<1, 2>>>(d_q, d->lines);
    G16_LAUNCH_CHECK();
    pairing_product_kernel<C><<<1, 1>>>(d_alpha, d_beta, 1, d_out, d->ab, d_status);
    G16_LAUNCH_CHECK();
    if (nb) {
        const uint64_t lanes = nb * WINDOWS * DIGITS;
        verify_window_table_kernel<C><<<(unsigned)((lanes + 127) / 128), 128>>>(d_bases, nb, d->tables);
        G16_LAUNCH_CHECK();
    }
    G16_HIP_TRY(hipDeviceSynchronize());
    int st = 0;
    G16_HIP_TRY(hipMemcpy(&st, d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) return G16_ERR_UNEXPECTED_IDENTITY;
    G16_HIP_TRY(hipMemcpy(ab_out, d_out, 12 * (C::Fq::N / 2) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return G16_OK;
}

template <class C>
int verify_chunk(hipStream_t s, const PvkDev<C>* d, const uint64_t* proofs, const uint64_t* inputs, uint64_t num_public,
                 const uint64_t* prepared, uint64_t n, uint8_t* verdicts, DevBufs& bufs) {
    constexpr int L = C::Fq::N / 2;
    G16_HIP_TRY(hipSetDevice(d->device));
    uint64_t *d_proofs, *d_inputs = nullptr, *d_prep = nullptr;
    uint8_t* d_v;
    G16_TRY(bufs.get(&d_proofs, n * 8 * L));
    G16_TRY(bufs.get(&d_v, n));
    G16_HIP_TRY(hipMemcpyAsync(d_proofs, proofs, n * 8 * L * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (prepared) {
        G16_TRY(bufs.get(&d_prep, n * 2 * L));
        G16_HIP_TRY(hipMemcpyAsync(d_prep, prepared, n * 2 * L * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    } else if (num_public) {
        G16_TRY(bufs.get(&d_inputs, n * num_public * 4));
        G16_HIP_TRY(hipMemcpyAsync(d_inputs, inputs, n * num_public * 4 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    }
    verify_batch_kernel<C><<<(unsigned)((n + VERIFY_BLOCK - 1) / VERIFY_BLOCK), VERIFY_BLOCK, 0, s>>>(
        d->lines, d->tables, d->ab, d->gabc0, d_proofs, d_inputs, num_public, d_prep, n, d->id_flags, d_v);
    G16_LAUNCH_CHECK();
    G16_HIP_TRY(hipMemcpyAsync(verdicts, d_v, n, hipMemcpyDeviceToHost, s));
    return G16_OK;
}

// one lane of the first device: the product of n_pairs pairings
template <class C>
int pairing_any(int device, const uint64_t* g1s, const uint64_t* g2s, uint64_t n_pairs, uint64_t* out) {
    constexpr int L = C::Fq::N / 2;
    G16_HIP_TRY(hipSetDevice(device));
    DevBufs bufs;
    uint64_t *d1, *d2, *dout;
    int* dst;
    G16_TRY(dev_upload(bufs, g1s, n_pairs * 2 * L, &d1));
    G16_TRY(dev_upload(bufs, g2s, n_pairs * 4 * L, &d2));
    G16_TRY(bufs.get(&dout, 12 * L));
    G16_TRY(bufs.get(&dst, 1));
    pairing_product_kernel<C><<<1, 1>>>(reinterpret_cast<const typename C::G1A*>(d1), reinterpret_cast<const typename C::G2A*>(d2), n_pairs, dout,
                                        nullptr, dst);
    G16_LAUNCH_CHECK();
    G16_HIP_TRY(hipDeviceSynchronize());
    int st = 0;
    G16_HIP_TRY(hipMemcpy(&st, dst, sizeof(int), hipMemcpyDeviceToHost));
    if (st) return G16_ERR_UNEXPECTED_IDENTITY;
    G16_HIP_TRY(hipMemcpy(out, dout, 12 * L * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return G16_OK;
}

template <class C>
int host_pairing(const uint64_t* g1s, const uint64_t* g2s, uint64_t n, uint64_t* out) {
    typename Pairing<C>::F12 e;
    if (!host_pairing_product<C>(g1s, g2s, n, e)) return G16_ERR_UNEXPECTED_IDENTITY;
    Pairing<C>::store_gt(e, out);
    return G16_OK;
}

template <class C>
int host_verify(const g16_vk_view* vk, const uint64_t* proof, const uint64_t* x, uint64_t num_public, uint8_t* verdict) {
    typedef Pairing<C> PP;
    typedef typename PP::F F;
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    constexpr int L = C::Fq::N / 2;
    const G1A A = ld<G1A>(proof);
    const G2A B = ld<G2A>(proof + 2 * L);
    const G1A Cc = ld<G1A>(proof + 6 * L);
    if (!PP::g1_on_curve(A) || !PP::g2_on_curve(B) || !PP::g1_on_curve(Cc)) { *verdict = 2; return G16_OK; }
    // IC = gamma_abc[0] + sum x_j gamma_abc[j + 1]  (variable-base here: the host form is for single proofs)
    XYZZ<F> acc = XYZZ<F>::identity();
    for (uint64_t j = 0; j <= num_public; ++j) {
        const G1A gj = ld<G1A>(vk->gamma_abc_g1 + j * 2 * L);
        if (gj.is_identity()) continue;
        const typename PP::A1 g = PP::g1_in(gj);
        XYZZ<F> t = XYZZ<F>::from_affine(Aff1<C>{g.x, g.y});
        if (j) {
            uint32_t k[8];
            ld<typename C::Fr>(x + (j - 1) * 4).to_canonical(k);
            t = t.mul_bits(k, 256);
        }
        acc.add(t);
    }
    const Aff1<C> ic = acc.to_affine();
    G1A ps[3] = {A, G1A::identity(), Cc};
    if (!ic.is_identity()) { ps[1].x = ic.x.to_std(); ps[1].y = ic.y.to_std(); }
    G2A qs[3] = {B, ld<G2A>(vk->gamma_g2), ld<G2A>(vk->delta_g2)};
    qs[1] = qs[1].neg();
    qs[2] = qs[2].neg();
    typename PP::LiveQ lq[3];
    typename PP::A1 pa[3];
    bool skip[3];
    const typename PP::F12 f = PP::miller_live(ps, qs, 3, lq, pa, skip);
    typename PP::F12 ef, eg;
    if (!PP::final_exp(f, ef)) { *verdict = 0; return G16_OK; }
    G16_TRY(host_alpha_beta<C>(vk, eg));
    *verdict = PP::equal(ef, eg) ? 1 : 0;
    return G16_OK;
}

}  // namespace g16

namespace {
template <class C>
int verify_any(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, const uint64_t* inputs, uint64_t num_public,
               const uint64_t* prepared, uint64_t n, uint8_t* verdicts) {
    constexpr int L = C::Fq::N / 2;
    CtxView cv;
    G16_TRY(cv.load(ctx));
    const std::vector<PvkDev<C>>& pd = devs_of<C>(const_cast<g16_pvk*>(pvk));
    if (pd.size() != cv.devs.size()) return G16_ERR_BAD_ARG;   // the key was loaded on another context
    return for_each_chunk(cv, n, [&](uint64_t k, uint64_t lo, uint64_t cnt, DevBufs& bufs) -> int {
        return verify_chunk<C>(cv.streams[k], &pd[k], proofs + lo * 8 * L, inputs ? inputs + lo * num_public * 4 : nullptr, num_public,
                               prepared ? prepared + lo * 2 * L : nullptr, cnt, verdicts + lo, bufs);
    });
}
}  // namespace

template <class C>
static int pvk_load_all(const CtxView& cv, const g16_vk_view* vk, g16_pvk** out) {
    const std::vector<int>& devs = cv.devs;
    g16_pvk* p = new g16_pvk();
    p->curve = cv.curve;
    p->n_gamma_abc = vk->n_gamma_abc;
    constexpr int L = C::Fq::N / 2;
    p->gamma_g2.assign(vk->gamma_g2, vk->gamma_g2 + 4 * L);
    p->delta_g2.assign(vk->delta_g2, vk->delta_g2 + 4 * L);
    p->gamma_abc_g1.assign(vk->gamma_abc_g1, vk->gamma_abc_g1 + vk->n_gamma_abc * 2 * L);
    std::vector<PvkDev<C>>& pd = devs_of<C>(p);
    pd.resize(devs.size());
    for (size_t k = 0; k < devs.size(); ++k) {
        const int rc = pvk_load_dev<C>(devs[k], vk, &pd[k], p->ab);
        if (rc != G16_OK) { delete p; return rc; }
    }
    *out = p;
    return G16_OK;
}

extern "C" {

int g16_pvk_load(g16_ctx* ctx, const g16_vk_view* vk, g16_pvk** out) {
    if (!ctx || !out || !vk_view_ok(vk)) return G16_ERR_BAD_ARG;
    CtxView cv;
    G16_TRY(cv.load(ctx));
    G16_VERIFY_DISPATCH(cv.curve, pvk_load_all<CC>(cv, vk, out));
}

void g16_pvk_free(g16_pvk* pvk) { delete pvk; }

int g16_pvk_alpha_beta(const g16_pvk* pvk, uint64_t* out_fq12) {
    if (!pvk || !out_fq12) return G16_ERR_BAD_ARG;
    memcpy(out_fq12, pvk->ab, 12 * (pvk->curve == G16_BLS12_381 ? 6 : 4) * sizeof(uint64_t));
    return G16_OK;
}

int g16_verify_batch(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, uint64_t n, const uint64_t* public_inputs,
                     uint64_t num_public, uint8_t* verdicts) {
    if (!ctx || !pvk || (n && (!proofs || !verdicts)) || (n && num_public && !public_inputs)) return G16_ERR_BAD_ARG;
    if (num_public + 1 != pvk->n_gamma_abc) return G16_ERR_MALFORMED_VK;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(pvk->curve, (verify_any<CC>(ctx, pvk, proofs, public_inputs, num_public, nullptr, n, verdicts)));
}

int g16_verify_batch_prepared(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* proofs, const uint64_t* prepared_inputs, uint64_t n,
                              uint8_t* verdicts) {
    if (!ctx || !pvk || (n && (!proofs || !prepared_inputs || !verdicts))) return G16_ERR_BAD_ARG;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(pvk->curve, (verify_any<CC>(ctx, pvk, proofs, nullptr, 0, prepared_inputs, n, verdicts)));
}

int g16_pairing(g16_ctx* ctx, const uint64_t* g1s, const uint64_t* g2s, uint64_t n_pairs, uint64_t* out_fq12) {
    if (!ctx || !out_fq12 || (n_pairs && (!g1s || !g2s))) return G16_ERR_BAD_ARG;
    CtxView cv;
    G16_TRY(cv.load(ctx));
    G16_VERIFY_DISPATCH(cv.curve, pairing_any<CC>(cv.devs[0], g1s, g2s, n_pairs, out_fq12));
}

int g16_host_pairing(int curve, const uint64_t* g1s, const uint64_t* g2s, uint64_t n_pairs, uint64_t* out_fq12) {
    if (!out_fq12 || (n_pairs && (!g1s || !g2s))) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(curve, host_pairing<CC>(g1s, g2s, n_pairs, out_fq12));
}

int g16_host_verify(int curve, const g16_vk_view* vk, const uint64_t* proof, const uint64_t* public_inputs, uint64_t num_public,
                    uint8_t* verdict) {
    if (!vk_view_ok(vk) || !proof || !verdict || (num_public && !public_inputs)) return G16_ERR_BAD_ARG;
    if (num_public + 1 != vk->n_gamma_abc) return G16_ERR_MALFORMED_VK;
    G16_VERIFY_DISPATCH(curve, host_verify<CC>(vk, proof, public_inputs, num_public, verdict));
}

}  // extern "C"
