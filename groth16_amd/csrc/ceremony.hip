// libg16_ceremony.so (include/g16_ceremony.h): is an SRS a sequence of powers, does a proving key descend from its predecessor
// (DESIGN.md 4.9).  A companion of libg16_mi355x.so, linked against it: this file holds the library's two kernels, the checks, their
// host twins and the entry points; the sort, the passes, the reductions, the membership launches and the pairing are the prover library's.
//
// Everything is a random linear combination with 128-bit coefficients rho_i.  For a point array X the pair
//     lo = sum_{i<n-1} rho_i X[i],   hi = sum_{i<n-1} rho_i X[i+1]
// satisfies e(lo, tau G2) == e(hi, G2) for every rho iff X[i+1] = tau X[i] for all i (with X in the prime-order subgroup a wrong
// array survives with probability <= 2^-128: the difference of the two sides is a non-zero linear form in the rho_i).  The sums are
// MSMs with SHORT scalars, so the pipeline is the prover's with a new front:
//   upload X once -> membership (verify_subgroup.hip's kernels, on that copy) -> ceremony_first_bad_kernel
//   -> ceremony_digits128_kernel + sort_digit_planes (msm_sort.hip: the per-window histogram / scatter) under coeffs128_plan: a plan over
//      128 bits, half the windows of Fr
//   -> convert_bases in place -> msm_bucket_pass_batch: lo and hi are the SAME sort read with shift 0 and shift 1, and every array of
//      one call shares that sort (a shorter array skips the entries beyond its end: the pass's base_count test)
//   -> msm_reduce_batch -> fold_windows on the host -> a two-pair pairing product per equation (host templates), compared with 1.
//
//   ceremony_digits128_kernel   one lane per coefficient: the two raw words ARE the canonical integer (no Montgomery reduction, no
//                               modulus compare); rho + K, at most 160 bits for c <= 16, staged in LDS as digits_kernel stages its
//                               words (each lane reads back only its own column: no barrier), W windows out as the same u16 planes.
//   ceremony_first_bad_kernel   one lane per point: the membership flag (2 off the curve, 0 outside the subgroup) or, where the
//                               identity is not allowed, the all-zero test of the point's words -> a reason; one ballot per wave, the
//                               wave's first bad lane takes a 64-bit atomic minimum of (array, index, reason) on one record in HBM.
//                               The minimum does not depend on the order the waves arrive in.  No LDS.
// The host twins (g16_host_*) run plain scalar multiplications and additions, Subgroup<C> and the host pairing.  The host helpers of
// the three companion libraries (stage timers, the stream wait, uploads, Grp, flag -> reason, the bad-point record, pairs_equal, refuse,
// the checks of an SRS view, the stage times as a timings struct) are ceremony_common.hpp's.
#include "ceremony_common.hpp"

using namespace g16;

namespace g16 {

constexpr int CEREMONY_BLOCK = 256;

struct DigitPlan {
    int c, W;
    uint32_t K[COEFF128_SWORDS - 1];   // the signed-digit bias (MsmPlan::K; zero beyond, checked by coeffs128_plan)
};
__global__ __launch_bounds__(256) void ceremony_digits128_kernel(const uint64_t* __restrict__ coeffs, uint64_t n, DigitPlan plan,
                                                                 uint16_t* __restrict__ planes) {
    __shared__ uint32_t sw[COEFF128_SWORDS][256];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t lo = coeffs[2 * i], hi = coeffs[2 * i + 1];
    const uint32_t s[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    uint64_t carry = 0;
    G16_UNROLL for (int k = 0; k < COEFF128_SWORDS - 1; ++k) {
        carry += (uint64_t)(k < 4 ? s[k] : 0u) + plan.K[k];
        sw[k][threadIdx.x] = (uint32_t)carry;
        carry >>= 32;
    }
    sw[COEFF128_SWORDS - 1][threadIdx.x] = 0;
    for (int w = 0; w < plan.W; ++w) {
        const int bit = w * plan.c, word = bit >> 5, sh = bit & 31;
        const uint64_t two = (uint64_t)sw[word][threadIdx.x] | ((uint64_t)sw[word + 1][threadIdx.x] << 32);
        planes[(uint64_t)w * n + i] = (uint16_t)((uint32_t)(two >> sh) & ((1u << plan.c) - 1u));
    }
}

// key = array << 48 | index << 8 | reason  (index < 2^31): bad_key's layout (ceremony_common.hpp), written out here for the device
__global__ __launch_bounds__(CEREMONY_BLOCK) void ceremony_first_bad_kernel(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ points,
                                                                           uint32_t words, uint64_t n, uint32_t array, uint32_t allow_identity,
                                                                           unsigned long long* __restrict__ rec) {
    const uint64_t i = (uint64_t)blockIdx.x * CEREMONY_BLOCK + threadIdx.x;
    uint32_t reason = 0;
    if (i < n) {
        const uint8_t f = flags[i];
        if (f == 2) reason = 2;
        else if (f == 0) reason = 3;
        else if (!allow_identity) {
            uint64_t any = 0;
            for (uint32_t w = 0; w < words; ++w) any |= points[i * words + w];
            if (!any) reason = 4;
        }
    }
    const unsigned long long m = __ballot(reason != 0);   // wave64: one bit per lane, indices ascend with the lane
    if (m == 0) return;
    if ((threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m) - 1))
        atomicMin(rec, ((unsigned long long)array << 48) | ((unsigned long long)i << 8) | reason);
}

namespace {

typedef StageTimes<g16_ceremony_timings, 6> Stages;
g16_ceremony_timings* tm_of(const CeremonyEnv& env) { return Stages::of(env.stage_ms); }

struct CallTimers {
    Timers upload, membership, sort, passes, reductions;
    double pairings = 0;
    void store(g16_ceremony_timings* tm) {
        tm->upload_ms = upload.total(); tm->membership_ms = membership.total(); tm->sort_ms = sort.total();
        tm->passes_ms = passes.total(); tm->reductions_ms = reductions.total(); tm->pairings_ms = pairings;
    }
};

// the membership kernels over one uploaded array, then its first bad point into the call's record
template <class C, int G2>
int enqueue_membership(const CeremonyEnv& env, const typename Grp<C, G2>::A* d_pts, uint64_t n, uint32_t array, bool allow_identity,
                       unsigned long long* d_rec) {
    if (!n) return G16_OK;
    uint8_t* d_flags = nullptr;
    G16_TRY(env.arena->alloc_n(n, &d_flags));
    const uint64_t* words = reinterpret_cast<const uint64_t*>(d_pts);
    G16_TRY(subgroup_enqueue_points(env.st, C::CURVE_ID, G2, words, n, d_flags));
    hipLaunchKernelGGL(ceremony_first_bad_kernel, dim3((unsigned)((n + CEREMONY_BLOCK - 1) / CEREMONY_BLOCK)), dim3(CEREMONY_BLOCK), 0, env.st,
                       d_flags, words, Grp<C, G2>::WORDS, n, array, allow_identity ? 1u : 0u, d_rec);
    G16_LAUNCH_CHECK();
    return G16_OK;
}

// host twin of the two stages above; true: a bad point was recorded (the first in call order wins: arrays are scanned in field order)
template <class C, int G2>
bool host_membership(const uint64_t* pts, uint64_t n, uint32_t array, bool allow_identity, unsigned long long* rec) {
    typedef typename Grp<C, G2>::A A;
    if (*rec != BAD_NONE) return true;
    for (uint64_t i = 0; i < n; ++i)
        if (const uint32_t reason = point_reason<C, G2>(ld_any<A>(pts + i * Grp<C, G2>::WORDS), allow_identity)) {
            *rec = bad_key(array, i, reason);
            return true;
        }
    return false;
}

// sum_{i < count} rho_i X[i + shift], plain double-and-add
template <class F>
Affine<F> host_sum(const uint64_t* pts, uint64_t count, uint64_t shift, const uint64_t* coeffs) {
    XYZZ<F> acc = XYZZ<F>::identity();
    constexpr size_t W = sizeof(Affine<F>) / sizeof(uint64_t);
    for (uint64_t i = 0; i < count; ++i) {
        uint32_t k[4];
        coeff_words(coeffs + 2 * i, k);
        acc.add(XYZZ<F>::from_affine(ld_any<Affine<F>>(pts + (i + shift) * W)).mul_bits(k, 128));
    }
    return acc.to_affine();
}

// one sum per job over the shared sort: the passes in batches of four (one launch each), their reductions, the fold on the host
template <class F>
struct SumJob {
    const Affine<F>* d_bases;   // in the bucket kernel's radix (convert_bases)
    int64_t shift;
    uint64_t base_count;
};
template <class F>
int run_sums(const CeremonyEnv& env, const ScalarSort& ss, const SumJob<F>* jobs, int njobs, Affine<F>* out, CallTimers& ct) {
    typedef XYZZ<F> X;
    const int outs = ss.plan.outputs();
    std::vector<X> hws((size_t)outs * njobs);
    std::vector<MsmBuffers<F>> bufs(njobs);
    for (int lo = 0; lo < njobs; lo += 4) {
        const int cnt = std::min(4, njobs - lo);
        PassJob<F> pj[4];
        const MsmBuffers<F>* bb[4];
        const ScalarSort* sp[4];
        for (int k = 0; k < cnt; ++k) {
            pj[k] = {jobs[lo + k].d_bases, jobs[lo + k].shift, jobs[lo + k].base_count, &ss, &bufs[lo + k]};
            bb[k] = &bufs[lo + k];
            sp[k] = &ss;
        }
        G16_TRY((msm_bucket_pass_batch<F>(pj, cnt, *env.arena, env.st, ct.passes.add())));
        EventTimer* tr = ct.reductions.add();
        G16_TRY(tr->start(env.st));
        G16_TRY((msm_reduce_batch<F>(bb, sp, cnt, env.st, false)));
        G16_TRY(tr->stop(env.st));
        for (int k = 0; k < cnt; ++k)
            G16_HIP_TRY(hipMemcpyAsync(hws.data() + (size_t)(lo + k) * outs, bufs[lo + k].window_sums, sizeof(X) * outs, hipMemcpyDeviceToHost,
                                       env.st));
    }
    G16_HIP_TRY(hipStreamSynchronize(env.st));
    for (int j = 0; j < njobs; ++j) out[j] = fold_windows<F>(hws.data() + (size_t)j * outs, ss.plan).to_affine();
    return G16_OK;
}

// the coefficients on the device and their sort
int sort_on_device(const CeremonyEnv& env, const uint64_t* rho, uint64_t m, ScalarSort* ss, CallTimers& ct) {
    uint64_t* d_rho = nullptr;
    G16_TRY(env.arena->alloc_n(2 * m, &d_rho));
    G16_HIP_TRY(hipMemcpyAsync(d_rho, rho, 2 * m * sizeof(uint64_t), hipMemcpyHostToDevice, env.st));
    EventTimer* t = ct.sort.add();
    G16_TRY(t->start(env.st));
    MsmPlan plan;
    G16_TRY(coeffs128_plan(m, &plan));
    DigitPlan dp;
    dp.c = plan.c; dp.W = plan.W;
    for (int k = 0; k < COEFF128_SWORDS - 1; ++k) dp.K[k] = plan.K[k];
    uint16_t* planes = nullptr;
    G16_TRY(env.arena->alloc_n(m * (uint64_t)plan.W, &planes));
    hipLaunchKernelGGL(ceremony_digits128_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, env.st, d_rho, m, dp, planes);
    G16_LAUNCH_CHECK();
    G16_TRY(sort_digit_planes(plan, planes, m, *env.arena, env.st, ss));
    G16_TRY(t->stop(env.st));
    if (env.window_bits) *env.window_bits = ss->plan.c;
    if (env.windows) *env.windows = ss->plan.W;
    return G16_OK;
}

template <class C, int G2>
int rlc_device(const CeremonyEnv& env, const uint64_t* points, uint64_t n, const uint64_t* rho, uint64_t* out_lo, uint64_t* out_hi) {
    typedef typename Grp<C, G2>::F F;
    CallTimers ct;
    StreamWait wait{env.st};
    Affine<F>* d_x = nullptr;
    EventTimer* tu = ct.upload.add();
    G16_TRY(tu->start(env.st));
    G16_TRY(upload(env, points, n, &d_x));
    G16_TRY(tu->stop(env.st));
    ScalarSort ss;
    G16_TRY(sort_on_device(env, rho, n - 1, &ss, ct));
    G16_TRY((convert_bases<F>(d_x, n, env.st)));
    const SumJob<F> jobs[2] = {{d_x, 0, n - 1}, {d_x, 1, n}};
    Affine<F> out[2];
    G16_TRY((run_sums<F>(env, ss, jobs, 2, out, ct)));
    memcpy(out_lo, &out[0], sizeof(Affine<F>));
    memcpy(out_hi, &out[1], sizeof(Affine<F>));
    ct.store(tm_of(env));
    return G16_OK;
}

}  // namespace

template <class C>
int rlc_sums_device(const CeremonyEnv& env, int g2, const uint64_t* points, uint64_t n, const uint64_t* coeffs, uint64_t* out_lo, uint64_t* out_hi) {
    *tm_of(env) = g16_ceremony_timings{};
    const size_t bytes = (g2 ? 2 : 1) * sizeof(typename C::G1A);
    if (n == 1) { memset(out_lo, 0, bytes); memset(out_hi, 0, bytes); return G16_OK; }
    std::vector<uint64_t> own;
    const uint64_t* rho = nullptr;
    G16_TRY(agg_coeffs(coeffs, n - 1, own, &rho));
    return g2 ? rlc_device<C, 1>(env, points, n, rho, out_lo, out_hi) : rlc_device<C, 0>(env, points, n, rho, out_lo, out_hi);
}

template <class C>
int rlc_sums_host(int g2, const uint64_t* points, uint64_t n, const uint64_t* coeffs, uint64_t* out_lo, uint64_t* out_hi) {
    std::vector<uint64_t> own;
    const uint64_t* rho = nullptr;
    G16_TRY(agg_coeffs(coeffs, n - 1, own, &rho));
    if (g2) {
        const typename C::G2A lo = host_sum<typename C::Fq2>(points, n - 1, 0, rho), hi = host_sum<typename C::Fq2>(points, n - 1, 1, rho);
        memcpy(out_lo, &lo, sizeof(lo));
        memcpy(out_hi, &hi, sizeof(hi));
    } else {
        const typename C::G1A lo = host_sum<typename C::Fq>(points, n - 1, 0, rho), hi = host_sum<typename C::Fq>(points, n - 1, 1, rho);
        memcpy(out_lo, &lo, sizeof(lo));
        memcpy(out_hi, &hi, sizeof(hi));
    }
    return G16_OK;
}

// ---- the SRS ----------------------------------------------------------------------------------------------------------------
namespace {
template <class C>
struct SrsSums {
    typename C::G1A g1[6];   // lo / hi of tau_g1, alpha_tau_g1, beta_tau_g1
    typename C::G2A g2[2];   // lo / hi of tau_g2
};

// *bad: the record of the first bad point (BAD_NONE: every point passed, and then `sums` is filled)
template <class C>
int srs_sums_device(const CeremonyEnv& env, const g16_srs_view* srs, const uint64_t* rho, uint64_t m, unsigned long long* bad, SrsSums<C>* sums,
                    CallTimers& ct) {
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    const uint64_t N1 = srs->n_tau_g1, N2 = srs->n_tau_g2, M = srs->n_alpha_beta;
    StreamWait wait{env.st};
    Affine<Fq>*d_t1 = nullptr, *d_a = nullptr, *d_b = nullptr;
    Affine<Fq2>*d_t2 = nullptr, *d_bg2 = nullptr;
    unsigned long long* d_rec = nullptr;
    EventTimer* tu = ct.upload.add();
    G16_TRY(tu->start(env.st));
    G16_TRY(upload(env, srs->tau_g1, N1, &d_t1));
    G16_TRY(upload(env, srs->tau_g2, N2, &d_t2));
    G16_TRY(upload(env, srs->alpha_tau_g1, M, &d_a));
    G16_TRY(upload(env, srs->beta_tau_g1, M, &d_b));
    G16_TRY(upload(env, srs->beta_g2, 1, &d_bg2));
    G16_TRY(tu->stop(env.st));
    G16_TRY(env.arena->alloc_n(1, &d_rec));
    G16_HIP_TRY(hipMemsetAsync(d_rec, 0xff, sizeof(unsigned long long), env.st));
    EventTimer* tm = ct.membership.add();
    G16_TRY(tm->start(env.st));
    G16_TRY((enqueue_membership<C, 0>(env, d_t1, N1, 0, false, d_rec)));
    G16_TRY((enqueue_membership<C, 1>(env, d_t2, N2, 1, false, d_rec)));
    G16_TRY((enqueue_membership<C, 0>(env, d_a, M, 2, false, d_rec)));
    G16_TRY((enqueue_membership<C, 0>(env, d_b, M, 3, false, d_rec)));
    G16_TRY((enqueue_membership<C, 1>(env, d_bg2, 1, 4, false, d_rec)));
    G16_TRY(tm->stop(env.st));
    G16_HIP_TRY(hipMemcpyAsync(bad, d_rec, sizeof(unsigned long long), hipMemcpyDeviceToHost, env.st));
    G16_HIP_TRY(hipStreamSynchronize(env.st));
    if (*bad != BAD_NONE) return G16_OK;
    ScalarSort ss;
    G16_TRY(sort_on_device(env, rho, m, &ss, ct));
    G16_TRY((convert_bases<Fq>(d_t1, N1, env.st)));
    G16_TRY((convert_bases<Fq2>(d_t2, N2, env.st)));
    G16_TRY((convert_bases<Fq>(d_a, M, env.st)));
    G16_TRY((convert_bases<Fq>(d_b, M, env.st)));
    // lo reads entry p at X[p] for p < N - 1, hi at X[p + 1] for p + 1 < N: the sort covers max(N) - 1 coefficients, a shorter array
    // skips the rest
    const SumJob<Fq> j1[6] = {{d_t1, 0, N1 - 1}, {d_t1, 1, N1}, {d_a, 0, M - 1}, {d_a, 1, M}, {d_b, 0, M - 1}, {d_b, 1, M}};
    const SumJob<Fq2> j2[2] = {{d_t2, 0, N2 - 1}, {d_t2, 1, N2}};
    G16_TRY((run_sums<Fq>(env, ss, j1, 6, sums->g1, ct)));
    G16_TRY((run_sums<Fq2>(env, ss, j2, 2, sums->g2, ct)));
    return G16_OK;
}

template <class C>
void srs_sums_host(const g16_srs_view* srs, const uint64_t* rho, unsigned long long* bad, SrsSums<C>* sums) {
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    const uint64_t N1 = srs->n_tau_g1, N2 = srs->n_tau_g2, M = srs->n_alpha_beta;
    *bad = BAD_NONE;
    if (host_membership<C, 0>(srs->tau_g1, N1, 0, false, bad) || host_membership<C, 1>(srs->tau_g2, N2, 1, false, bad) ||
        host_membership<C, 0>(srs->alpha_tau_g1, M, 2, false, bad) || host_membership<C, 0>(srs->beta_tau_g1, M, 3, false, bad) ||
        host_membership<C, 1>(srs->beta_g2, 1, 4, false, bad))
        return;
    sums->g1[0] = host_sum<Fq>(srs->tau_g1, N1 - 1, 0, rho);
    sums->g1[1] = host_sum<Fq>(srs->tau_g1, N1 - 1, 1, rho);
    sums->g1[2] = host_sum<Fq>(srs->alpha_tau_g1, M - 1, 0, rho);
    sums->g1[3] = host_sum<Fq>(srs->alpha_tau_g1, M - 1, 1, rho);
    sums->g1[4] = host_sum<Fq>(srs->beta_tau_g1, M - 1, 0, rho);
    sums->g1[5] = host_sum<Fq>(srs->beta_tau_g1, M - 1, 1, rho);
    sums->g2[0] = host_sum<Fq2>(srs->tau_g2, N2 - 1, 0, rho);
    sums->g2[1] = host_sum<Fq2>(srs->tau_g2, N2 - 1, 1, rho);
}
}  // namespace

template <class C>
int srs_check_any(const CeremonyEnv* env, const g16_srs_view* srs, const uint64_t* coeffs, g16_ceremony_info* info) {
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    constexpr uint32_t W1 = Grp<C, 0>::WORDS, W2 = Grp<C, 1>::WORDS;
    *info = g16_ceremony_info{};
    if (env) *tm_of(*env) = g16_ceremony_timings{};
    const uint64_t N1 = srs->n_tau_g1, N2 = srs->n_tau_g2, M = srs->n_alpha_beta;
    const uint64_t m = std::max(std::max(N1, N2), M) - 1;
    std::vector<uint64_t> own;
    const uint64_t* rho = nullptr;
    G16_TRY(agg_coeffs(coeffs, m, own, &rho));
    SrsSums<C> s;
    unsigned long long bad = BAD_NONE;
    CallTimers ct;
    if (env) {
        const int rc = srs_sums_device<C>(*env, srs, rho, m, &bad, &s, ct);
        ct.store(tm_of(*env));
        G16_TRY(rc);
    } else {
        srs_sums_host<C>(srs, rho, &bad, &s);
    }
    if (bad != BAD_NONE) { decode_bad(bad, G16_SRS_BAD_POINT, info); return G16_OK; }
    const G1A g1 = ld_any<G1A>(srs->tau_g1), tau1 = ld_any<G1A>(srs->tau_g1 + W1), beta1 = ld_any<G1A>(srs->beta_tau_g1);
    const G2A g2 = ld_any<G2A>(srs->tau_g2), tau2 = ld_any<G2A>(srs->tau_g2 + W2), beta2 = ld_any<G2A>(srs->beta_g2);
    const double t0 = wall_ms();
    uint32_t flags = 0;
    bool eq = true;
    G16_TRY(pairs_equal<C>(s.g1[0], tau2, s.g1[1], g2, &eq));
    if (!eq) flags |= G16_SRS_TAU_G1;
    G16_TRY(pairs_equal<C>(tau1, s.g2[0], g1, s.g2[1], &eq));
    if (!eq) flags |= G16_SRS_TAU_G2;
    if (M >= 2) {
        G16_TRY(pairs_equal<C>(s.g1[2], tau2, s.g1[3], g2, &eq));
        if (!eq) flags |= G16_SRS_ALPHA;
        G16_TRY(pairs_equal<C>(s.g1[4], tau2, s.g1[5], g2, &eq));
        if (!eq) flags |= G16_SRS_BETA;
    }
    G16_TRY(pairs_equal<C>(beta1, g2, g1, beta2, &eq));
    if (!eq) flags |= G16_SRS_BETA_G2;
    if (env) tm_of(*env)->pairings_ms = wall_ms() - t0;
    info->flags = flags;
    return G16_OK;
}

// ---- a delta contribution ------------------------------------------------------------------------------------------------------
namespace {
// the first differing point of two arrays of n points of `words` 64-bit words; n if none
uint64_t first_difference(const uint64_t* a, const uint64_t* b, uint64_t n, uint32_t words) {
    for (uint64_t i = 0; i < n; ++i)
        if (memcmp(a + i * words, b + i * words, words * sizeof(uint64_t)) != 0) return i;
    return n;
}

template <class C>
int key_sums_device(const CeremonyEnv& env, const g16_params_view* before, const g16_params_view* after, uint64_t n_l, uint64_t n_h,
                    const uint64_t* rho, uint64_t m, unsigned long long* bad, typename C::G1A sums[4], CallTimers& ct) {
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    StreamWait wait{env.st};
    Affine<Fq>*d_d1 = nullptr, *d_al = nullptr, *d_ah = nullptr, *d_bl = nullptr, *d_bh = nullptr;
    Affine<Fq2>* d_d2 = nullptr;
    unsigned long long* d_rec = nullptr;
    EventTimer* tu = ct.upload.add();
    G16_TRY(tu->start(env.st));
    G16_TRY(upload(env, after->delta_g1, 1, &d_d1));
    G16_TRY(upload(env, after->delta_g2, 1, &d_d2));
    G16_TRY(upload(env, after->l_query, n_l, &d_al));
    G16_TRY(upload(env, after->h_query, n_h, &d_ah));
    G16_TRY(upload(env, before->l_query, n_l, &d_bl));
    G16_TRY(upload(env, before->h_query, n_h, &d_bh));
    G16_TRY(tu->stop(env.st));
    G16_TRY(env.arena->alloc_n(1, &d_rec));
    G16_HIP_TRY(hipMemsetAsync(d_rec, 0xff, sizeof(unsigned long long), env.st));
    EventTimer* tm = ct.membership.add();
    G16_TRY(tm->start(env.st));
    G16_TRY((enqueue_membership<C, 0>(env, d_d1, 1, 0, false, d_rec)));
    G16_TRY((enqueue_membership<C, 1>(env, d_d2, 1, 1, false, d_rec)));
    G16_TRY((enqueue_membership<C, 0>(env, d_al, n_l, 2, true, d_rec)));
    G16_TRY((enqueue_membership<C, 0>(env, d_ah, n_h, 3, true, d_rec)));
    G16_TRY(tm->stop(env.st));
    G16_HIP_TRY(hipMemcpyAsync(bad, d_rec, sizeof(unsigned long long), hipMemcpyDeviceToHost, env.st));
    G16_HIP_TRY(hipStreamSynchronize(env.st));
    if (*bad != BAD_NONE || !m) return G16_OK;
    ScalarSort ss;
    G16_TRY(sort_on_device(env, rho, m, &ss, ct));
    G16_TRY((convert_bases<Fq>(d_al, n_l, env.st)));
    G16_TRY((convert_bases<Fq>(d_ah, n_h, env.st)));
    G16_TRY((convert_bases<Fq>(d_bl, n_l, env.st)));
    G16_TRY((convert_bases<Fq>(d_bh, n_h, env.st)));
    const SumJob<Fq> jobs[4] = {{d_al, 0, n_l}, {d_bl, 0, n_l}, {d_ah, 0, n_h}, {d_bh, 0, n_h}};   // one batch, one launch
    return run_sums<Fq>(env, ss, jobs, 4, sums, ct);
}
}  // namespace

template <class C>
int params_check_delta_any(const CeremonyEnv* env, const g16_params_view* before, const g16_params_view* after, uint64_t n_vars, uint64_t n_inputs,
                           uint64_t n_l, uint64_t n_h, const uint64_t* coeffs, g16_ceremony_info* info) {
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    typedef typename C::Fq Fq;
    constexpr uint32_t W1 = Grp<C, 0>::WORDS, W2 = Grp<C, 1>::WORDS;
    *info = g16_ceremony_info{};
    if (env) *tm_of(*env) = g16_ceremony_timings{};
    const uint64_t m = std::max(n_l, n_h);
    std::vector<uint64_t> own;
    const uint64_t* rho = nullptr;
    G16_TRY(agg_coeffs(coeffs, m, own, &rho));
    G1A sums[4] = {G1A::identity(), G1A::identity(), G1A::identity(), G1A::identity()};   // after.l, before.l, after.h, before.h
    unsigned long long bad = BAD_NONE;
    CallTimers ct;
    if (env) {
        const int rc = key_sums_device<C>(*env, before, after, n_l, n_h, rho, m, &bad, sums, ct);
        ct.store(tm_of(*env));
        G16_TRY(rc);
    } else if (!host_membership<C, 0>(after->delta_g1, 1, 0, false, &bad) && !host_membership<C, 1>(after->delta_g2, 1, 1, false, &bad) &&
               !host_membership<C, 0>(after->l_query, n_l, 2, true, &bad) && !host_membership<C, 0>(after->h_query, n_h, 3, true, &bad)) {
        sums[0] = host_sum<Fq>(after->l_query, n_l, 0, rho);
        sums[1] = host_sum<Fq>(before->l_query, n_l, 0, rho);
        sums[2] = host_sum<Fq>(after->h_query, n_h, 0, rho);
        sums[3] = host_sum<Fq>(before->h_query, n_h, 0, rho);
    }
    if (bad != BAD_NONE) { decode_bad(bad, G16_KEY_BAD_POINT, info); return G16_OK; }
    uint32_t flags = 0;
    // the part no contribution may touch: a host compare, the first difference in field order
    const struct { const uint64_t *a, *b; uint64_t n; uint32_t words; } fixed[8] = {
        {before->alpha_g1, after->alpha_g1, 1, W1},          {before->beta_g1, after->beta_g1, 1, W1},
        {before->beta_g2, after->beta_g2, 1, W2},            {before->gamma_g2, after->gamma_g2, 1, W2},
        {before->gamma_abc_g1, after->gamma_abc_g1, n_inputs, W1}, {before->a_query, after->a_query, n_vars, W1},
        {before->b_g1_query, after->b_g1_query, n_vars, W1}, {before->b_g2_query, after->b_g2_query, n_vars, W2}};
    for (uint32_t k = 0; k < 8; ++k) {
        const uint64_t i = first_difference(fixed[k].a, fixed[k].b, fixed[k].n, fixed[k].words);
        if (i < fixed[k].n) {
            flags |= G16_KEY_FIXED_PART;
            info->bad_array = k;
            info->bad_index = i;
            break;
        }
    }
    const G1A bd1 = ld_any<G1A>(before->delta_g1), ad1 = ld_any<G1A>(after->delta_g1);
    const G2A bd2 = ld_any<G2A>(before->delta_g2), ad2 = ld_any<G2A>(after->delta_g2);
    const double t0 = wall_ms();
    bool eq = true;
    G16_TRY(pairs_equal<C>(ad1, bd2, bd1, ad2, &eq));
    if (!eq) flags |= G16_KEY_DELTA;
    if (n_l) {
        G16_TRY(pairs_equal<C>(sums[0], ad2, sums[1], bd2, &eq));
        if (!eq) flags |= G16_KEY_L;
    }
    if (n_h) {
        G16_TRY(pairs_equal<C>(sums[2], ad2, sums[3], bd2, &eq));
        if (!eq) flags |= G16_KEY_H;
    }
    if (env) tm_of(*env)->pairings_ms = wall_ms() - t0;
    info->flags = flags;
    return G16_OK;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
namespace {
// what both forms of g16_srs_check refuse alike: every array long enough for one equation, enough explicit coefficients
int srs_args(const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs) {
    if (!srs_view_ok(srs)) return G16_ERR_BAD_ARG;
    const SrsArray arr[] = {{"tau_g1", srs->n_tau_g1, 2}, {"tau_g2", srs->n_tau_g2, 2}, {"alpha_tau_g1 / beta_tau_g1", srs->n_alpha_beta, 1}};
    G16_TRY(srs_lengths(arr, "SRS check: %s holds %llu points, the check needs %llu", 0, "SRS check: %s holds 2^31 points or more"));
    const uint64_t longest = std::max(std::max(srs->n_tau_g1, srs->n_tau_g2), srs->n_alpha_beta);
    if (coeffs && n_coeffs < longest - 1)
        return refuse(G16_ERR_BAD_LENGTH, "SRS check%s: %llu coefficients, the longest array (%llu points) needs %llu", n_coeffs, longest, longest - 1);
    return G16_OK;
}

int key_args(const g16_params_view* before, const g16_params_view* after, uint64_t n_vars, uint64_t n_inputs, uint64_t n_l, uint64_t n_h,
             const uint64_t* coeffs, uint64_t n_coeffs) {
    for (const g16_params_view* v : {before, after}) {
        if (!v->alpha_g1 || !v->beta_g1 || !v->delta_g1 || !v->beta_g2 || !v->delta_g2 || !v->gamma_g2) return G16_ERR_BAD_ARG;
        if (v->flags & G16_PARAMS_DEVICE_PTRS) return G16_ERR_BAD_ARG;
        if ((n_inputs && !v->gamma_abc_g1) || (n_vars && (!v->a_query || !v->b_g1_query || !v->b_g2_query))) return G16_ERR_BAD_ARG;
        if ((n_l && !v->l_query) || (n_h && !v->h_query)) return G16_ERR_BAD_ARG;
    }
    if (n_l >= ((uint64_t)1 << 31) || n_h >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
    if (coeffs && n_coeffs < std::max(n_l, n_h))
        return refuse(G16_ERR_BAD_LENGTH, "key check%s: %llu coefficients, l_query / h_query hold %llu / %llu points", n_coeffs, n_l, n_h);
    return G16_OK;
}
}  // namespace

}  // namespace g16

extern "C" {

int g16_rlc_plan(uint64_t n_coeffs, uint32_t out[4]) {
    if (!out) return G16_ERR_BAD_ARG;
    MsmPlan plan;
    G16_TRY(coeffs128_plan(n_coeffs, &plan));
    out[0] = (uint32_t)plan.c; out[1] = (uint32_t)plan.W; out[2] = plan.chunk; out[3] = plan.Lmax;
    return G16_OK;
}

int g16_rlc_sums(g16_ctx* ctx, int g2, const uint64_t* points, uint64_t n, const uint64_t* coeffs, uint64_t* out_lo, uint64_t* out_hi) {
    if (!ctx || (g2 != 0 && g2 != 1) || !points || !n || !out_lo || !out_hi) return G16_ERR_BAD_ARG;
    if (n >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    G16_VERIFY_DISPATCH(curve, (rlc_sums_device<CC>(env, g2, points, n, coeffs, out_lo, out_hi)));
}

int g16_host_rlc_sums(int curve, int g2, const uint64_t* points, uint64_t n, const uint64_t* coeffs, uint64_t* out_lo, uint64_t* out_hi) {
    if ((g2 != 0 && g2 != 1) || !points || !n || !out_lo || !out_hi) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(curve, (rlc_sums_host<CC>(g2, points, n, coeffs, out_lo, out_hi)));
}

int g16_srs_check(g16_ctx* ctx, const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    if (!ctx || !srs || !info) return G16_ERR_BAD_ARG;
    G16_TRY(srs_args(srs, coeffs, n_coeffs));
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    G16_VERIFY_DISPATCH(curve, (srs_check_any<CC>(&env, srs, coeffs, info)));
}

int g16_host_srs_check(int curve, const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    if (!srs || !info) return G16_ERR_BAD_ARG;
    G16_TRY(srs_args(srs, coeffs, n_coeffs));
    G16_VERIFY_DISPATCH(curve, (srs_check_any<CC>(nullptr, srs, coeffs, info)));
}

int g16_params_check_delta(g16_ctx* ctx, const g16_params_view* before, const g16_params_view* after, uint64_t n_vars, uint64_t n_inputs,
                           uint64_t n_l, uint64_t n_h, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    if (!ctx || !before || !after || !info) return G16_ERR_BAD_ARG;
    G16_TRY(key_args(before, after, n_vars, n_inputs, n_l, n_h, coeffs, n_coeffs));
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    G16_VERIFY_DISPATCH(curve, (params_check_delta_any<CC>(&env, before, after, n_vars, n_inputs, n_l, n_h, coeffs, info)));
}

int g16_host_params_check_delta(int curve, const g16_params_view* before, const g16_params_view* after, uint64_t n_vars, uint64_t n_inputs,
                                uint64_t n_l, uint64_t n_h, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    if (!before || !after || !info) return G16_ERR_BAD_ARG;
    G16_TRY(key_args(before, after, n_vars, n_inputs, n_l, n_h, coeffs, n_coeffs));
    G16_VERIFY_DISPATCH(curve, (params_check_delta_any<CC>(nullptr, before, after, n_vars, n_inputs, n_l, n_h, coeffs, info)));
}

int g16_ceremony_get_timings(g16_ctx* ctx, g16_ceremony_timings* out) {
    return Stages::get(ceremony_stage_ms(ctx), out);
}

}  // extern "C"
