// libg16_phase1.so (include/g16_phase1.h): phase 1 of a setup ceremony -- contribute to a powers-of-tau SRS, check a contribution
// (DESIGN.md 4.10).  A companion of libg16_mi355x.so and libg16_ceremony.so, linked against both: this file holds the library's two
// kernels, the contribution, the check, their host twins and the entry points.
//
//   batch_scalar_mul_kernel   out[i] = k_i P_i, one lane per G1 point, a lane pair per G2 point (scalar_mul.hpp: fixed signed 4-bit
//                             window, XYZZ in the 30-bit lazy arithmetic, the table 1P .. 8P and the biased scalar parked
//                             limb-planar in HBM, wave-uniform control flow, one inversion per point).
//   phase1_powers_kernel      out[i] = s tau^(first + i): a lane raises tau to the first index of its run, then steps through the
//                             run.  The output feeds the kernel above on the device; it is the toxic waste and never leaves it.
// A contribution walks each array in chunks: upload, powers, multiply in place, download; the scalar buffer and the park buffer are
// zeroed on the stream before the call returns.  The check is g16_srs_check on `after` plus three two-pair products on the host.
// The stage timers, the stream wait, Grp, the reason of a bad point, pairs_equal and the stage times are ceremony_common.hpp's.
#include "ceremony_common.hpp"
#include "../../include/g16_phase1.h"
#include "scalar_mul.hpp"
#include "scalar_mul_host.hpp"
#include <algorithm>
#include <cstdlib>

using namespace g16;

namespace g16 {

constexpr int SMUL_THREADS = 128;
constexpr uint64_t PHASE1_CHUNK_DEFAULT = (uint64_t)1 << 17;   // points per launch: the park buffer is <= 445 MB (G2, 13 limbs)
constexpr uint64_t PHASE1_RUN_DEFAULT = 16, PHASE1_RUN_MAX = 1024;

template <class F30, class Fr>
__global__ __launch_bounds__(SMUL_THREADS, 2) void batch_scalar_mul_kernel(const Affine<typename F30::Std>* pts, const Fr* __restrict__ scalars,
                                                                           uint64_t count, Affine<typename F30::Std>* out,
                                                                           uint32_t* __restrict__ park) {
    typedef SmulDeviceIO<F30> IO;
    typedef typename IO::W32 W32;
    static_assert(Fr::N == SMUL_KWORDS, "a scalar is eight 32-bit words");
    static_assert(Fr::Params::mod(SMUL_KWORDS - 1) < 0x77777777u, "r + 0x88..8 must fit 256 bits: 64 signed digits, no carry out");
    const uint64_t lane = (uint64_t)blockIdx.x * SMUL_THREADS + threadIdx.x;
    const uint64_t t = lane / F30::LANES_PER_TASK;   // lanes of one task are adjacent
    if (t >= count) return;
    const uint64_t stride = count * F30::LANES_PER_TASK;
    uint32_t* kpark = park + (uint64_t)SMUL_SLOTS * IO::NL * stride + lane;
    {
        uint32_t k[SMUL_KWORDS], kb[SMUL_KWORDS];
        scalars[t].to_canonical(k);
        (void)smul_bias(k, kb);
        G16_UNROLL for (int w = 0; w < SMUL_KWORDS; ++w) kpark[(uint64_t)w * stride] = kb[w];
    }
    IO io{reinterpret_cast<const W32*>(pts + t), reinterpret_cast<W32*>(out + t), park + lane, kpark, stride};
    scalar_mul_task<F30>(io);
}

template <class Fr>
__global__ __launch_bounds__(64) void phase1_powers_kernel(Fr tau, Fr scale, uint64_t first, uint64_t n, uint32_t run, Fr* __restrict__ out) {
    const uint64_t lo = ((uint64_t)blockIdx.x * 64 + threadIdx.x) * run;
    if (lo >= n) return;
    const uint64_t hi = lo + run < n ? lo + run : n;
    Fr v = scale * tau.pow_u64(first + lo);
    for (uint64_t i = lo; i < hi; ++i) {
        out[i] = v;
        v = v * tau;
    }
}

namespace {

template <class F> struct Lazy;
template <class P> struct Lazy<Fp<P>> { typedef Fp30<P> type; };
template <class P> struct Lazy<Fp2<P>> { typedef Fp2p30<P> type; };

typedef StageTimes<g16_phase1_timings, 5> Stages;

uint64_t env_u64(const char* name, uint64_t dflt, uint64_t lo, uint64_t hi) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    return std::min(std::max<uint64_t>(strtoull(e, nullptr, 10), lo), hi);
}
uint64_t phase1_chunk() { return env_u64("G16_PHASE1_CHUNK", PHASE1_CHUNK_DEFAULT, 1, (uint64_t)1 << 22); }
uint32_t phase1_run() { return (uint32_t)env_u64("G16_PHASE1_RUN", PHASE1_RUN_DEFAULT, 1, PHASE1_RUN_MAX); }

template <class F>
size_t park_words(uint64_t count) {
    typedef typename Lazy<F>::type F30;
    return (size_t)(SMUL_SLOTS * TableLane<F30>::B::NL + SMUL_KWORDS) * count * F30::LANES_PER_TASK;
}

struct CallTimers {
    Timers upload, powers, mul[2], download;
    void store(g16_phase1_timings* tm) {
        tm->upload_ms = upload.total(); tm->powers_ms = powers.total(); tm->mul_g1_ms = mul[0].total(); tm->mul_g2_ms = mul[1].total();
        tm->download_ms = download.total();
    }
};
// the buffers of one call; wipe() queues their zeroing (the scalars and the biased scalars in the park buffer are secrets)
struct Work {
    void* pts = nullptr;
    void* scalars = nullptr;
    uint32_t* park = nullptr;
    size_t pts_bytes = 0, scalar_bytes = 0, park_bytes = 0;
    template <class C>
    int alloc(const CeremonyEnv& env, uint64_t chunk, bool g2) {
        pts_bytes = chunk * (g2 ? sizeof(typename C::G2A) : sizeof(typename C::G1A));
        scalar_bytes = chunk * sizeof(typename C::Fr);
        park_bytes = sizeof(uint32_t) * (g2 ? park_words<typename C::Fq2>(chunk) : park_words<typename C::Fq>(chunk));
        G16_TRY(env.arena->alloc(pts_bytes, &pts));
        G16_TRY(env.arena->alloc(scalar_bytes, &scalars));
        G16_TRY(env.arena->alloc(park_bytes, (void**)&park));
        return G16_OK;
    }
    int wipe(hipStream_t st) const {
        G16_HIP_TRY(hipMemsetAsync(scalars, 0, scalar_bytes, st));
        G16_HIP_TRY(hipMemsetAsync(park, 0, park_bytes, st));
        return G16_OK;
    }
};
// every exit wipes and waits: kernels in flight read arena memory that the next call reuses and write the caller's arrays.  The order
// is the language's: this destructor's body queues the wipes, then the member `wait` is destroyed and waits for them
struct WipeAndWait {
    const Work& w;
    StreamWait wait;
    ~WipeAndWait() { if (w.scalars) (void)w.wipe(wait.s); }
};

template <class C, int G2>
int launch_mul(const CeremonyEnv& env, const Work& w, uint64_t count, CallTimers& ct) {
    typedef typename Grp<C, G2>::F F;
    typedef typename Lazy<F>::type F30;
    typedef typename C::Fr Fr;
    static_assert(sizeof(Affine<F>) == 2 * TableLane<F30>::PARTS * sizeof(typename TableLane<F30>::B::Std), "affine point = x parts | y parts");
    const uint64_t lanes = count * F30::LANES_PER_TASK;
    EventTimer* t = ct.mul[G2].add();
    G16_TRY(t->start(env.st));
    hipLaunchKernelGGL((batch_scalar_mul_kernel<F30, Fr>), dim3((unsigned)((lanes + SMUL_THREADS - 1) / SMUL_THREADS)), dim3(SMUL_THREADS), 0, env.st,
                       static_cast<const Affine<F>*>(w.pts), static_cast<const Fr*>(w.scalars), count, static_cast<Affine<F>*>(w.pts), w.park);
    G16_LAUNCH_CHECK();
    G16_TRY(t->stop(env.st));
    return G16_OK;
}

template <class C, int G2>
int copy_in(const CeremonyEnv& env, const Work& w, const uint64_t* host, uint64_t count, CallTimers& ct) {
    EventTimer* t = ct.upload.add();
    G16_TRY(t->start(env.st));
    G16_HIP_TRY(hipMemcpyAsync(w.pts, host, count * Grp<C, G2>::WORDS * sizeof(uint64_t), hipMemcpyHostToDevice, env.st));
    G16_TRY(t->stop(env.st));
    return G16_OK;
}
template <class C, int G2>
int copy_out(const CeremonyEnv& env, const Work& w, uint64_t* host, uint64_t count, CallTimers& ct) {
    EventTimer* t = ct.download.add();
    G16_TRY(t->start(env.st));
    G16_HIP_TRY(hipMemcpyAsync(host, w.pts, count * Grp<C, G2>::WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, env.st));
    G16_TRY(t->stop(env.st));
    return G16_OK;
}

template <class C, int G2>
int batch_mul_device(const CeremonyEnv& env, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out, CallTimers& ct) {
    typedef typename C::Fr Fr;
    const uint64_t chunk = std::min(n, phase1_chunk());
    Work w;
    G16_TRY(w.alloc<C>(env, chunk, G2 != 0));
    WipeAndWait guard{w, {env.st}};
    for (uint64_t first = 0; first < n; first += chunk) {
        const uint64_t count = std::min(chunk, n - first);
        G16_TRY((copy_in<C, G2>(env, w, points + first * Grp<C, G2>::WORDS, count, ct)));
        G16_HIP_TRY(hipMemcpyAsync(w.scalars, scalars + first * (sizeof(Fr) / sizeof(uint64_t)), count * sizeof(Fr), hipMemcpyHostToDevice, env.st));
        G16_TRY((launch_mul<C, G2>(env, w, count, ct)));
        G16_TRY((copy_out<C, G2>(env, w, out + first * Grp<C, G2>::WORDS, count, ct)));
    }
    G16_HIP_TRY(hipStreamSynchronize(env.st));
    return G16_OK;
}

// array[i] <- scale tau^(first_power + i) array[i], i < n, in place
template <class C, int G2>
int contribute_array(const CeremonyEnv& env, const Work& w, uint64_t chunk, uint32_t run, uint64_t* array, uint64_t n, const typename C::Fr& tau,
                     const typename C::Fr& scale, uint64_t first_power, CallTimers& ct) {
    typedef typename C::Fr Fr;
    for (uint64_t first = 0; first < n; first += chunk) {
        const uint64_t count = std::min(chunk, n - first);
        uint64_t* host = array + first * Grp<C, G2>::WORDS;
        G16_TRY((copy_in<C, G2>(env, w, host, count, ct)));
        EventTimer* t = ct.powers.add();
        G16_TRY(t->start(env.st));
        const uint64_t lanes = (count + run - 1) / run;
        hipLaunchKernelGGL((phase1_powers_kernel<Fr>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, env.st, tau, scale, first_power + first, count,
                           run, static_cast<Fr*>(w.scalars));
        G16_LAUNCH_CHECK();
        G16_TRY(t->stop(env.st));
        G16_TRY((launch_mul<C, G2>(env, w, count, ct)));
        G16_TRY((copy_out<C, G2>(env, w, host, count, ct)));
    }
    return G16_OK;
}

template <class F, class Fr>
Affine<F> host_mul(const Affine<F>& p, const Fr& k) {
    uint32_t w[Fr::N];
    k.to_canonical(w);
    return XYZZ<F>::from_affine(p).mul_bits(w, 32 * Fr::N).to_affine();
}

template <class C>
struct Secrets {
    typename C::Fr tau, alpha, beta;
    int load(const uint64_t* t, const uint64_t* a, const uint64_t* b) {
        memcpy(&tau, t, sizeof(tau)); memcpy(&alpha, a, sizeof(alpha)); memcpy(&beta, b, sizeof(beta));
        return (tau.is_zero() || alpha.is_zero() || beta.is_zero()) ? G16_ERR_UNEXPECTED_IDENTITY : G16_OK;
    }
};

// the parts both forms run on the host: the public record from the OLD g2, then beta_g2
template <class C>
void contribute_singles(const Secrets<C>& s, const g16_srs_view* io, const g16_tau_contribution* pub) {
    typedef typename C::G2A G2A;
    const G2A g2 = ld_any<G2A>(io->tau_g2);
    const G2A pt = host_mul(g2, s.tau), pa = host_mul(g2, s.alpha), pb = host_mul(g2, s.beta);
    memcpy(pub->tau_g2, &pt, sizeof(G2A)); memcpy(pub->alpha_g2, &pa, sizeof(G2A)); memcpy(pub->beta_g2, &pb, sizeof(G2A));
    const G2A b2 = host_mul(ld_any<G2A>(io->beta_g2), s.beta);
    memcpy(io->beta_g2, &b2, sizeof(G2A));
}

}  // namespace

template <class C>
int batch_scalar_mul_any(const CeremonyEnv* env, int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out,
                         g16_phase1_timings* tm) {
    typedef typename C::Fr Fr;
    if (env) {
        CallTimers ct;
        const int rc = g2 ? batch_mul_device<C, 1>(*env, points, scalars, n, out, ct) : batch_mul_device<C, 0>(*env, points, scalars, n, out, ct);
        if (rc == G16_OK) ct.store(tm);
        return rc;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const Fr k = ld_any<Fr>(scalars + i * (sizeof(Fr) / sizeof(uint64_t)));
        if (g2) {
            const typename C::G2A r = host_mul(ld_any<typename C::G2A>(points + i * Grp<C, 1>::WORDS), k);
            memcpy(out + i * Grp<C, 1>::WORDS, &r, sizeof(r));
        } else {
            const typename C::G1A r = host_mul(ld_any<typename C::G1A>(points + i * Grp<C, 0>::WORDS), k);
            memcpy(out + i * Grp<C, 0>::WORDS, &r, sizeof(r));
        }
    }
    return G16_OK;
}

// ---- the device kernel's task on the host (the `not gpu` tests): scalar_mul_host.hpp ----------------------------------------------
template <class C>
int batch_scalar_mul_windowed_host(int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out) {
    typedef typename C::Fr Fr;
    typedef typename C::Fq::Params QP;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t k[SMUL_KWORDS];
        ld_any<Fr>(scalars + i * (sizeof(Fr) / sizeof(uint64_t))).to_canonical(k);
        if (g2) {
            typedef Fp2h30<QP> F;
            const typename C::G2A p = ld_any<typename C::G2A>(points + i * Grp<C, 1>::WORDS);
            SmulHostIO<F> io;
            if (!smul_bias(k, io.kb)) return G16_ERR_INTERNAL;
            io.finite = !p.is_identity();
            io.x0 = F{in30(p.x.c0), in30(p.x.c1)};
            io.y0 = F{in30(p.y.c0), in30(p.y.c1)};
            scalar_mul_task<F>(io);
            typename C::G2A r = C::G2A::identity();
            if (!io.oid) r = {{io.ox.c0.to_std(), io.ox.c1.to_std()}, {io.oy.c0.to_std(), io.oy.c1.to_std()}};
            memcpy(out + i * Grp<C, 1>::WORDS, &r, sizeof(r));
        } else {
            typedef Fp30<QP> F;
            const typename C::G1A p = ld_any<typename C::G1A>(points + i * Grp<C, 0>::WORDS);
            SmulHostIO<F> io;
            if (!smul_bias(k, io.kb)) return G16_ERR_INTERNAL;
            io.finite = !p.is_identity();
            io.x0 = in30(p.x);
            io.y0 = in30(p.y);
            scalar_mul_task<F>(io);
            typename C::G1A r = C::G1A::identity();
            if (!io.oid) r = {io.ox.to_std(), io.oy.to_std()};
            memcpy(out + i * Grp<C, 0>::WORDS, &r, sizeof(r));
        }
    }
    return G16_OK;
}

// ---- a contribution -----------------------------------------------------------------------------------------------------------
template <class C>
int srs_contribute_any(const CeremonyEnv* env, const uint64_t* tau_, const uint64_t* alpha_, const uint64_t* beta_, const g16_srs_view* io,
                       const g16_tau_contribution* pub, g16_phase1_timings* tm) {
    typedef typename C::Fr Fr;
    Secrets<C> s;
    G16_TRY(s.load(tau_, alpha_, beta_));
    const uint64_t N1 = io->n_tau_g1, N2 = io->n_tau_g2, M = io->n_alpha_beta;
    constexpr uint32_t W1 = Grp<C, 0>::WORDS, W2 = Grp<C, 1>::WORDS;
    contribute_singles<C>(s, io, pub);   // reads tau_g2[0], which no later step writes
    if (env) {
        const uint64_t longest = std::max(std::max(N1, N2), M);
        const uint64_t chunk = std::max<uint64_t>(std::min(longest, phase1_chunk()), 1);
        const uint32_t run = phase1_run();
        CallTimers ct;
        Work w;
        G16_TRY(w.alloc<C>(*env, chunk, true));
        int rc;
        {
            WipeAndWait guard{w, {env->st}};
            auto body = [&]() -> int {
                G16_TRY((contribute_array<C, 0>(*env, w, chunk, run, io->tau_g1 + W1, N1 - 1, s.tau, Fr::one(), 1, ct)));
                G16_TRY((contribute_array<C, 1>(*env, w, chunk, run, io->tau_g2 + W2, N2 - 1, s.tau, Fr::one(), 1, ct)));
                G16_TRY((contribute_array<C, 0>(*env, w, chunk, run, io->alpha_tau_g1, M, s.tau, s.alpha, 0, ct)));
                G16_TRY((contribute_array<C, 0>(*env, w, chunk, run, io->beta_tau_g1, M, s.tau, s.beta, 0, ct)));
                return G16_OK;
            };
            rc = body();
        }
        if (rc == G16_OK) ct.store(tm);
        return rc;
    }
    auto scale = [&](uint64_t* arr, uint64_t n, uint64_t first, const Fr& sc, bool g2) {
        Fr k = sc;
        for (uint64_t i = 0; i < first; ++i) k = k * s.tau;
        for (uint64_t i = first; i < n; ++i, k = k * s.tau) {
            if (g2) {
                const typename C::G2A r = host_mul(ld_any<typename C::G2A>(arr + i * W2), k);
                memcpy(arr + i * W2, &r, sizeof(r));
            } else {
                const typename C::G1A r = host_mul(ld_any<typename C::G1A>(arr + i * W1), k);
                memcpy(arr + i * W1, &r, sizeof(r));
            }
        }
    };
    scale(io->tau_g1, N1, 1, Fr::one(), false);
    scale(io->tau_g2, N2, 1, Fr::one(), true);
    scale(io->alpha_tau_g1, M, 0, s.alpha, false);
    scale(io->beta_tau_g1, M, 0, s.beta, false);
    return G16_OK;
}

// ---- the check of a contribution ----------------------------------------------------------------------------------------------
template <class C>
int srs_check_contribution_any(g16_ctx* ctx, const g16_srs_view* before, const g16_srs_view* after, const g16_tau_contribution* pub,
                               const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    constexpr uint32_t W1 = Grp<C, 0>::WORDS, W2 = Grp<C, 1>::WORDS;
    // `after` as a whole: every point, every array a sequence of powers
    G16_TRY(ctx ? g16_srs_check(ctx, after, coeffs, n_coeffs, info) : g16_host_srs_check(C::CURVE_ID, after, coeffs, n_coeffs, info));
    if (info->flags & G16_SRS_BAD_POINT) return G16_OK;
    const G2A p2[3] = {ld_any<G2A>(pub->tau_g2), ld_any<G2A>(pub->alpha_g2), ld_any<G2A>(pub->beta_g2)};
    const G1A b_g1 = ld_any<G1A>(before->tau_g1), b_tau1 = ld_any<G1A>(before->tau_g1 + W1), b_alpha = ld_any<G1A>(before->alpha_tau_g1),
              b_beta = ld_any<G1A>(before->beta_tau_g1);
    const G2A b_g2 = ld_any<G2A>(before->tau_g2);
    auto bad = [&](uint32_t array, uint64_t index, uint32_t reason) {
        *info = g16_ceremony_info{};
        decode_bad(bad_key(array, index, reason), G16_TAU_BAD_POINT, info);
        return G16_OK;
    };
    for (uint32_t k = 0; k < 3; ++k)
        if (const uint32_t r = point_reason<C, 1>(p2[k], false)) return bad(5 + k, 0, r);
    if (const uint32_t r = point_reason<C, 0>(b_g1, false)) return bad(8, 0, r);
    if (const uint32_t r = point_reason<C, 0>(b_tau1, false)) return bad(8, 1, r);
    if (const uint32_t r = point_reason<C, 1>(b_g2, false)) return bad(8, 2, r);
    if (const uint32_t r = point_reason<C, 0>(b_alpha, false)) return bad(8, 3, r);
    if (const uint32_t r = point_reason<C, 0>(b_beta, false)) return bad(8, 4, r);
    uint32_t flags = info->flags;
    if (before->n_tau_g1 != after->n_tau_g1 || before->n_tau_g2 != after->n_tau_g2 || before->n_alpha_beta != after->n_alpha_beta ||
        memcmp(before->tau_g1, after->tau_g1, sizeof(G1A)) != 0 || memcmp(before->tau_g2, after->tau_g2, sizeof(G2A)) != 0)
        flags |= G16_TAU_SHAPE;
    bool eq = true;
    G16_TRY(pairs_equal<C>(ld_any<G1A>(after->tau_g1 + W1), b_g2, b_tau1, p2[0], &eq));
    if (!eq) flags |= G16_TAU_RATIO;
    G16_TRY(pairs_equal<C>(ld_any<G1A>(after->alpha_tau_g1), b_g2, b_alpha, p2[1], &eq));
    if (!eq) flags |= G16_TAU_ALPHA_RATIO;
    G16_TRY(pairs_equal<C>(ld_any<G1A>(after->beta_tau_g1), b_g2, b_beta, p2[2], &eq));
    if (!eq) flags |= G16_TAU_BETA_RATIO;
    info->flags = flags;
    return G16_OK;
}

namespace {
int unit_args(int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, const uint64_t* out) {
    if (g2 != 0 && g2 != 1) return G16_ERR_BAD_ARG;
    if (n && (!points || !scalars || !out)) return G16_ERR_BAD_ARG;
    if (n >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
    return G16_OK;
}
int contribute_args(const uint64_t* tau, const uint64_t* alpha, const uint64_t* beta, const g16_srs_view* io, const g16_tau_contribution* pub) {
    if (!tau || !alpha || !beta || !io || !pub || !pub->tau_g2 || !pub->alpha_g2 || !pub->beta_g2) return G16_ERR_BAD_ARG;
    if (!srs_view_ok(io)) return G16_ERR_BAD_ARG;
    if (io->n_tau_g1 < 1 || io->n_tau_g2 < 1) return G16_ERR_BAD_LENGTH;
    if (io->n_tau_g1 >= ((uint64_t)1 << 31) || io->n_tau_g2 >= ((uint64_t)1 << 31) || io->n_alpha_beta >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
    return G16_OK;
}
int check_args(const g16_srs_view* before, const g16_srs_view* after, const g16_tau_contribution* pub, const g16_ceremony_info* info) {
    if (!before || !after || !pub || !info || !pub->tau_g2 || !pub->alpha_g2 || !pub->beta_g2) return G16_ERR_BAD_ARG;
    if (!before->tau_g1 || !before->tau_g2 || !before->alpha_tau_g1 || !before->beta_tau_g1) return G16_ERR_BAD_ARG;
    if (before->n_tau_g1 < 2 || before->n_tau_g2 < 1 || before->n_alpha_beta < 1) {
        set_last_error_text("contribution check: `before` needs tau_g1[0], tau_g1[1], tau_g2[0], alpha_tau_g1[0] and beta_tau_g1[0]");
        return G16_ERR_BAD_LENGTH;
    }
    return G16_OK;
}
}  // namespace

}  // namespace g16

extern "C" {

int g16_batch_scalar_mul(g16_ctx* ctx, int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out) {
    if (!ctx) return G16_ERR_BAD_ARG;
    G16_TRY(unit_args(g2, points, scalars, n, out));
    if (!n) return G16_OK;
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    g16_phase1_timings* tm = Stages::of(phase1_stage_ms(ctx));
    *tm = g16_phase1_timings{};
    G16_VERIFY_DISPATCH(curve, (batch_scalar_mul_any<CC>(&env, g2, points, scalars, n, out, tm)));
}

int g16_host_batch_scalar_mul(int curve, int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out) {
    G16_TRY(unit_args(g2, points, scalars, n, out));
    G16_VERIFY_DISPATCH(curve, (batch_scalar_mul_any<CC>(nullptr, g2, points, scalars, n, out, nullptr)));
}

int g16_host_batch_scalar_mul_windowed(int curve, int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out) {
    G16_TRY(unit_args(g2, points, scalars, n, out));
    G16_VERIFY_DISPATCH(curve, (batch_scalar_mul_windowed_host<CC>(g2, points, scalars, n, out)));
}

int g16_srs_contribute(g16_ctx* ctx, const uint64_t tau[4], const uint64_t alpha[4], const uint64_t beta[4], const g16_srs_view* inout,
                       const g16_tau_contribution* pub, g16_phase1_timings* tm) {
    if (!ctx) return G16_ERR_BAD_ARG;
    G16_TRY(contribute_args(tau, alpha, beta, inout, pub));
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    g16_phase1_timings* kept = Stages::of(phase1_stage_ms(ctx));
    *kept = g16_phase1_timings{};
    int rc = G16_ERR_BAD_ARG;
    try {
        if (curve == G16_BLS12_381) rc = srs_contribute_any<Bls12_381>(&env, tau, alpha, beta, inout, pub, kept);
        else if (curve == G16_BN254) rc = srs_contribute_any<Bn254>(&env, tau, alpha, beta, inout, pub, kept);
    } catch (const std::bad_alloc&) {
        rc = G16_ERR_OOM;
    }
    if (tm) *tm = *kept;
    return rc;
}

int g16_host_srs_contribute(int curve, const uint64_t tau[4], const uint64_t alpha[4], const uint64_t beta[4], const g16_srs_view* inout,
                            const g16_tau_contribution* pub, g16_phase1_timings* tm) {
    G16_TRY(contribute_args(tau, alpha, beta, inout, pub));
    if (tm) *tm = g16_phase1_timings{};
    G16_VERIFY_DISPATCH(curve, (srs_contribute_any<CC>(nullptr, tau, alpha, beta, inout, pub, nullptr)));
}

int g16_phase1_get_timings(g16_ctx* ctx, g16_phase1_timings* out) {
    return Stages::get(phase1_stage_ms(ctx), out);
}

int g16_srs_check_contribution(g16_ctx* ctx, const g16_srs_view* before, const g16_srs_view* after, const g16_tau_contribution* pub,
                               const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    if (!ctx) return G16_ERR_BAD_ARG;
    G16_TRY(check_args(before, after, pub, info));
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    G16_VERIFY_DISPATCH(curve, (srs_check_contribution_any<CC>(ctx, before, after, pub, coeffs, n_coeffs, info)));
}

int g16_host_srs_check_contribution(int curve, const g16_srs_view* before, const g16_srs_view* after, const g16_tau_contribution* pub,
                                    const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    G16_TRY(check_args(before, after, pub, info));
    G16_VERIFY_DISPATCH(curve, (srs_check_contribution_any<CC>(nullptr, before, after, pub, coeffs, n_coeffs, info)));
}

}  // extern "C"
