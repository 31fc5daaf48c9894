// libg16_lagrange.so (include/g16_lagrange.h): the Lagrange form of a powers-of-tau SRS, made once per domain, and a circuit's key from
// it.  A companion of libg16_mi355x.so, libg16_ceremony.so and libg16_phase1.so: this file holds the library's three
// kernels, the transform over them, the preparation, the derivation from its result, their host twins and the entry points.
//
//   lagrange_addsub_kernel         s = a + b, d = a - b of a Gentleman-Sande butterfly, AFFINE in and out: both share the denominator
//                                  x_b - x_a, so one inversion gives both.  One lane per G1 butterfly, a lane pair per G2 one.
//   lagrange_twiddle_mul_kernel    d <- w d through scalar_mul_task (scalar_mul.hpp): phase 1's digits, table, selections and vote.
//                                  The twiddle comes from the power table, times the scale at stage 0 of an inverse transform.
//   lagrange_bitrev_kernel         out[i] = in[bitrev(i)]: the stages leave the bit-reversed order.
// Values travel AFFINE between stages (the reason is in DESIGN.md 4.12): every stage's output is canonical, and the primitive's affine
// load and store stay as they are.  Butterflies with twiddle 1 -- k = 0 of every block, all of the last stage -- take no
// multiplication: the multiplication kernel is launched over the others alone, so a wave never mixes the two kinds.
// g16_group_ntt multiplies by min(w, r - w) and negates: for a point outside the prime-order subgroup that is NOT w times the point
// (r P != O), so the same choice is made here -- bit-equality with that call is the contract.
#include "ceremony_common.hpp"
#include "../../include/g16_lagrange.h"
#include "scalar_mul.hpp"
#include "scalar_mul_host.hpp"
#include "srs_setup.hpp"
#include <algorithm>
#include <cstdlib>

using namespace g16;

namespace g16 {

constexpr int LAG_THREADS = 128;
constexpr uint64_t LAGRANGE_CHUNK_DEFAULT = (uint64_t)1 << 17;   // butterflies per launch: the park buffer is <= 445 MB (G2, 13 limbs)
constexpr int LAG_LINEAR = 40;   // a half_log above every count: butterfly t reads a[t] and b[t]
enum { LAG_MUL_SCALE = 1,        // stage 0 of an inverse transform: the twiddle times the scale, k = 0 included
       LAG_MUL_SUM = 2 };        // the same stage's sums: the scale alone

// butterfly t of a stage over blocks of 2^(half_log + 1): the index of its a (its b is half a block further)
G16_HD uint64_t lag_index(uint64_t t, int half_log) {
    return ((t >> half_log) << (half_log + 1)) + (t & (((uint64_t)1 << half_log) - 1));
}

// ---- the butterfly's sum and difference: the arithmetic of one task, written once for the device and for the host emulation -----
// IO: load_a / load_b (canonical coordinates in the R' radix; false for the identity), store_s / store_d (lazy coordinates < 16p),
// is_zero / select as in scalar_mul.hpp.  a = b, a = -b, an identity on either side and y = 0 are selections between the formula's
// result and the operands; no lane branches on its own data (is_zero votes per wave before its exact comparison).
//   x_a != x_b:  l = (+-y_b - y_a) / (x_b - x_a), the chord to b (the sum) and to -b (the difference): ONE denominator for both
//   x_a == x_b:  l = 3 x_a^2 / (2 y_a), the tangent at a, for whichever of the two is 2 a (a = b: the sum; a = -b: the difference);
//                the other one is the identity, and so are both when y_a = 0 (a = b = -b)
//   x = l^2 - x_a - x_b,  y = l (x_a - x) - y_a    in every case
// Bounds (multiples of p, per component): the inputs are canonical; dx, dy < 3; y_a + y_b < 2, its negative <= 4; 3 x_a^2 < 4.5; the
// denominator is passed through one product so that the inversion sees what it is proven for (< 1.5); l < 1.5; x < 5.5; x_a - x < 9;
// y < 3.5.
template <class F, class IO>
G16_HD void lagrange_addsub_task(IO& io) {
    F x1, y1, x2, y2;
    const bool fa = io.load_a(x1, y1), fb = io.load_b(x2, y2);
    const F dx = x2.template sub<2>(x1);
    const F dy = y2.template sub<2>(y1);
    const F sy = y1.add(y2);
    const bool same_x = io.is_zero(dx) && fa && fb;   // a = +-b
    const bool y_eq = io.is_zero(dy), y_opp = io.is_zero(sy);
    const F X2 = x1.sqr();
    const F M = X2.dbl().add(X2);
    const F den = io.select(same_x, y1.dbl(), dx).mul(F::one());
    const F inv = batch_inverse(den);   // y_a = 0 (a point of order two): zero, and the double is the identity below
    const F xx = x1.add(x2);
    const F nsy = F::zero().template sub<4>(sy);
    const F ls = io.select(same_x, M, dy).mul(inv);
    const F xs = ls.sqr().template sub<4>(xx);
    const F ys = ls.template mul_sub_k<2>(x1.template sub<8>(xs), y1);
    const F ld = io.select(same_x, M, nsy).mul(inv);
    const F xd = ld.sqr().template sub<4>(xx);
    const F yd = ld.template mul_sub_k<2>(x1.template sub<8>(xd), y1);
    const F ny2 = F::zero().template sub<2>(y2);
    const bool none = !fa && !fb;
    io.store_s(io.select(fa, io.select(fb, xs, x1), x2), io.select(fa, io.select(fb, ys, y1), y2), none || (same_x && y_opp));
    io.store_d(io.select(fa, io.select(fb, xd, x1), x2), io.select(fa, io.select(fb, yd, y1), ny2), none || (same_x && y_eq));
}

// the twiddle as the multiplication takes it: min(w, r - w) biased (smul_bias); true if r - w was taken and the product is negated
template <class Fr>
G16_HD bool lagrange_twiddle(const Fr& w, uint32_t kb[SMUL_KWORDS]) {
    uint32_t c[SMUL_KWORDS], d[SMUL_KWORDS];
    w.to_canonical(c);
    w.neg().to_canonical(d);
    bool neg = false, decided = false;
    G16_UNROLL for (int i = SMUL_KWORDS - 1; i >= 0; --i) {
        const bool differ = c[i] != d[i] && !decided;
        neg = differ ? d[i] < c[i] : neg;
        decided = decided || differ;
    }
    G16_UNROLL for (int i = 0; i < SMUL_KWORDS; ++i) c[i] = neg ? d[i] : c[i];
    (void)smul_bias(c, kb);
    return neg;
}

// ---- device side ------------------------------------------------------------------------------------------------------------------
// the two operands of a butterfly through the primitive's own affine load and store (a -> s, b -> d); s may be null: the sum is not kept
template <class F30>
struct LagAddSubIO {
    typedef SmulDeviceIO<F30> P;
    P pa, pb;
    G16_HD bool load_a(F30& x, F30& y) const { return pa.load(x, y); }
    G16_HD bool load_b(F30& x, F30& y) const { return pb.load(x, y); }
    G16_HD bool is_zero(const F30& v) const { return pa.is_zero(v); }
    G16_HD F30 select(bool c, const F30& a, const F30& b) const { return pa.select(c, a, b); }
    G16_HD void store_s(const F30& x, const F30& y, bool identity) const { if (pa.dst) pa.store(x, y, identity); }
    G16_HD void store_d(const F30& x, const F30& y, bool identity) const { pb.store(x, y, identity); }
};
// the primitive's IO with the product negated on the way out (identity: all zero either way)
template <class F30>
struct LagMulIO : SmulDeviceIO<F30> {
    typedef SmulDeviceIO<F30> P;
    typedef typename P::TL TL;
    typedef typename P::W32 W32;
    bool neg;
    G16_HD void store(const F30& x, const F30& y, bool identity) const {
        const int k = TL::part();
        const W32 xs = TL::comp(x).to_std(), ys = TL::comp(y).to_std(), yn = ys.neg();
        this->dst[k] = identity ? W32::zero() : xs;
        this->dst[TL::PARTS + k] = identity ? W32::zero() : neg ? yn : ys;
    }
};

// butterflies first .. first + count - 1 of a stage: a[i], b[i] -> s[i], d[i], i = lag_index(t, half_log); s may be null
template <class F30>
__global__ __launch_bounds__(LAG_THREADS, 2) void lagrange_addsub_kernel(const Affine<typename F30::Std>* a, const Affine<typename F30::Std>* b,
                                                                         Affine<typename F30::Std>* s, Affine<typename F30::Std>* d, uint64_t first,
                                                                         uint64_t count, int half_log) {
    typedef typename SmulDeviceIO<F30>::W32 W32;
    const uint64_t lane = (uint64_t)blockIdx.x * LAG_THREADS + threadIdx.x;
    const uint64_t j = lane / F30::LANES_PER_TASK;   // lanes of one task are adjacent
    if (j >= count) return;
    const uint64_t i = lag_index(first + j, half_log);
    LagAddSubIO<F30> io{{reinterpret_cast<const W32*>(a + i), s ? reinterpret_cast<W32*>(s + i) : nullptr, nullptr, nullptr, 0},
                        {reinterpret_cast<const W32*>(b + i), reinterpret_cast<W32*>(d + i), nullptr, nullptr, 0}};
    lagrange_addsub_task<F30>(io);
}

// multiplications first .. first + count - 1 of a stage, in place on pts[lag_index(t, half_log)].  Without a flag the u-th
// multiplication is that of the u-th butterfly whose k is not zero, by tw[k << tw_shift]; LAG_MUL_SCALE: of butterfly u, by
// tw[k << tw_shift] * scale; LAG_MUL_SUM: of butterfly u, by scale.  park: SMUL_SLOTS * NL + SMUL_KWORDS words per lane of the launch
template <class F30, class Fr>
__global__ __launch_bounds__(LAG_THREADS, 2) void lagrange_twiddle_mul_kernel(Affine<typename F30::Std>* pts, const Fr* __restrict__ tw, Fr scale,
                                                                              uint64_t first, uint64_t count, int half_log, int tw_shift, int flags,
                                                                              uint32_t* __restrict__ park) {
    typedef LagMulIO<F30> IO;
    typedef typename IO::W32 W32;
    static_assert(Fr::N == SMUL_KWORDS, "a scalar is eight 32-bit words");
    static_assert(Fr::Params::mod(SMUL_KWORDS - 1) < 0x77777777u, "r + 0x88..8 must fit 256 bits: 64 signed digits, no carry out");
    const uint64_t lane = (uint64_t)blockIdx.x * LAG_THREADS + threadIdx.x;
    const uint64_t j = lane / F30::LANES_PER_TASK;
    if (j >= count) return;
    const uint64_t stride = count * F30::LANES_PER_TASK;
    const uint64_t u = first + j, per = half_log ? ((uint64_t)1 << half_log) - 1 : 1;   // (half_log = 0 has no k but zero: never launched unflagged)
    const uint64_t t = flags ? u : ((u / per) << half_log) + 1 + u % per;
    const uint64_t e = (t & (((uint64_t)1 << half_log) - 1)) << tw_shift;
    const Fr w = (flags & LAG_MUL_SUM) ? scale : (flags & LAG_MUL_SCALE) ? tw[e] * scale : tw[e];
    uint32_t* kpark = park + (uint64_t)SMUL_SLOTS * IO::NL * stride + lane;
    bool neg;
    {
        uint32_t kb[SMUL_KWORDS];
        neg = lagrange_twiddle(w, kb);
        G16_UNROLL for (int x = 0; x < SMUL_KWORDS; ++x) kpark[(uint64_t)x * stride] = kb[x];
    }
    W32* p = reinterpret_cast<W32*>(pts + lag_index(t, half_log));
    IO io{{p, p, park + lane, kpark, stride}, neg};
    scalar_mul_task<F30>(io);
}

template <class A>
__global__ __launch_bounds__(64) void lagrange_bitrev_kernel(const A* __restrict__ in, int bits, A* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    out[i] = in[__brevll(i) >> (64 - bits)];   // (bits >= 1: a single point is copied by the host)
}

namespace {

template <class F> struct Lazy;
template <class P> struct Lazy<Fp<P>> { typedef Fp30<P> type; typedef Fp30<P> host; };
template <class P> struct Lazy<Fp2<P>> { typedef Fp2p30<P> type; typedef Fp2h30<P> host; };

typedef StageTimes<g16_lagrange_timings, 6> Stages;

uint64_t lagrange_chunk() {
    const char* e = getenv("G16_LAGRANGE_CHUNK");
    if (!e || !*e) return LAGRANGE_CHUNK_DEFAULT;
    return std::min(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), (uint64_t)1 << 22);
}

template <class C>
typename C::Fr root_of(int log_n) {
    typename C::Fr w = C::two_adic_root();
    for (int k = log_n; k < C::TWO_ADICITY; ++k) w = w.sqr();
    return w;
}
// tw[e] = base^e, e < count: the power table of the transforms of srs_setup.hip
template <class Fr>
std::vector<Fr> power_table(const Fr& base, uint64_t count) {
    std::vector<Fr> tw(count ? count : 1);
    Fr p = Fr::one();
    for (auto& x : tw) { x = p; p = p * base; }
    return tw;
}

// ---- the stages on the device -------------------------------------------------------------------------------------------------------
template <class C, int G2>
struct Dev {
    typedef typename Grp<C, G2>::F F;
    typedef typename Lazy<F>::type F30;
    typedef typename C::Fr Fr;
    typedef Affine<F> A;
    static_assert(sizeof(A) == 2 * TableLane<F30>::PARTS * sizeof(typename TableLane<F30>::B::Std), "affine point = x parts | y parts");
    static constexpr uint64_t LPT = F30::LANES_PER_TASK;

    static size_t park_words(uint64_t tasks) { return (size_t)(SMUL_SLOTS * TableLane<F30>::B::NL + SMUL_KWORDS) * tasks * LPT; }
    static unsigned blocks(uint64_t tasks) { return (unsigned)((tasks * LPT + LAG_THREADS - 1) / LAG_THREADS); }

    static int addsub(hipStream_t st, const A* a, const A* b, A* s, A* d, uint64_t first, uint64_t count, int half_log) {
        hipLaunchKernelGGL((lagrange_addsub_kernel<F30>), dim3(blocks(count)), dim3(LAG_THREADS), 0, st, a, b, s, d, first, count, half_log);
        G16_LAUNCH_CHECK();
        return G16_OK;
    }
    static int mul(hipStream_t st, A* pts, const Fr* d_tw, const Fr& scale, uint64_t first, uint64_t count, int half_log, int tw_shift, int flags,
                   uint32_t* park) {
        hipLaunchKernelGGL((lagrange_twiddle_mul_kernel<F30, Fr>), dim3(blocks(count)), dim3(LAG_THREADS), 0, st, pts, d_tw, scale, first, count,
                           half_log, tw_shift, flags, park);
        G16_LAUNCH_CHECK();
        return G16_OK;
    }
    // one stage over `count` butterflies of d (in place), in chunks.  odd_only: the sums are not kept (stage 0 of the Circom h
    // transform).  A chunk's multiplications follow its sums and differences on the stream; park holds `chunk` tasks
    static int stage(hipStream_t st, A* d, uint64_t count, int half_log, const Fr* d_tw, int tw_shift, bool scaled, const Fr& scale, bool odd_only,
                     uint64_t chunk, uint32_t* park) {
        const uint64_t half = (uint64_t)1 << half_log;
        for (uint64_t t0 = 0; t0 < count; t0 += chunk) {
            const uint64_t t1 = std::min(count, t0 + chunk);
            G16_TRY(addsub(st, d, d + half, odd_only ? nullptr : d, d + half, t0, t1 - t0, half_log));
            if (scaled) {
                if (!odd_only) G16_TRY(mul(st, d, d_tw, scale, t0, t1 - t0, half_log, tw_shift, LAG_MUL_SUM, park));
                G16_TRY(mul(st, d + half, d_tw, scale, t0, t1 - t0, half_log, tw_shift, LAG_MUL_SCALE, park));
            } else {
                // the butterflies below t whose k is not zero: t minus the multiples of half below t
                const uint64_t u0 = t0 - (t0 + half - 1) / half, u1 = t1 - (t1 + half - 1) / half;
                if (u1 > u0) G16_TRY(mul(st, d + half, d_tw, scale, u0, u1 - u0, half_log, tw_shift, 0, park));
            }
        }
        return G16_OK;
    }
    // the 2^log_n-point transform of d (in place, natural -> bit-reversed); d_tw[e << tw_extra] is the transform's root^e
    static int stages(hipStream_t st, A* d, int log_n, const Fr* d_tw, int tw_extra, bool scaled, const Fr& scale, uint64_t chunk, uint32_t* park) {
        const uint64_t count = ((uint64_t)1 << log_n) >> 1;
        for (int s = 0; s < log_n; ++s)
            G16_TRY(stage(st, d, count, log_n - 1 - s, d_tw, s + tw_extra, scaled && s == 0, scale, false, chunk, park));
        return G16_OK;
    }
    static int bitrev(hipStream_t st, const A* in, int log_n, A* out) {
        const uint64_t n = (uint64_t)1 << log_n;
        if (!log_n) {
            G16_HIP_TRY(hipMemcpyAsync(out, in, sizeof(A), hipMemcpyDeviceToDevice, st));
            return G16_OK;
        }
        hipLaunchKernelGGL((lagrange_bitrev_kernel<A>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, in, log_n, out, n);
        G16_LAUNCH_CHECK();
        return G16_OK;
    }
    // host[0 .. n) -> the inverse transform with n^-1 -> out_host[0 .. n); work, rev: n points each
    static int lagrange_array(const CeremonyEnv& env, const uint64_t* host, int log_n, const Fr* d_tw, int tw_extra, A* work, A* rev, uint64_t chunk,
                              uint32_t* park, uint64_t* out_host, EventTimer& tm) {
        const uint64_t n = (uint64_t)1 << log_n;
        G16_TRY(tm.start(env.st));
        G16_HIP_TRY(hipMemcpyAsync(work, host, n * sizeof(A), hipMemcpyHostToDevice, env.st));
        G16_TRY(stages(env.st, work, log_n, d_tw, tw_extra, true, Fr::from_u64(n).inverse(), chunk, park));
        G16_TRY(bitrev(env.st, work, log_n, rev));
        G16_HIP_TRY(hipMemcpyAsync(out_host, rev, n * sizeof(A), hipMemcpyDeviceToHost, env.st));
        G16_TRY(tm.stop(env.st));
        return G16_OK;
    }
};

// ---- the same on the host: one butterfly, one multiplication ---------------------------------------------------------------------------
template <class P> Fp30<P> to30(const Fp<P>& v) { return in30(v); }
template <class P> Fp2h30<P> to30(const Fp2<P>& v) { return {in30(v.c0), in30(v.c1)}; }
template <class P> Fp<P> from30(const Fp30<P>& v) { return v.to_std(); }
template <class P> Fp2<P> from30(const Fp2h30<P>& v) { return {v.c0.to_std(), v.c1.to_std()}; }

template <class F>
struct LagHostIO {
    typedef typename Lazy<F>::host H;
    Affine<F> a, b, s, d;
    static bool load(const Affine<F>& p, H& x, H& y) { x = to30(p.x); y = to30(p.y); return !p.is_identity(); }
    bool load_a(H& x, H& y) const { return load(a, x, y); }
    bool load_b(H& x, H& y) const { return load(b, x, y); }
    bool is_zero(const H& v) const { return zero30(v); }
    H select(bool c, const H& x, const H& y) const { return c ? x : y; }
    static Affine<F> out(const H& x, const H& y, bool identity) { return identity ? Affine<F>::identity() : Affine<F>{from30(x), from30(y)}; }
    void store_s(const H& x, const H& y, bool identity) { s = out(x, y, identity); }
    void store_d(const H& x, const H& y, bool identity) { d = out(x, y, identity); }
};

template <class F, class Fr>
int host_twiddle_mul(Affine<F>& p, const Fr& w) {
    typedef typename Lazy<F>::host H;
    SmulHostIO<H> io;
    const bool neg = lagrange_twiddle(w, io.kb);
    io.finite = !p.is_identity();
    io.x0 = to30(p.x);
    io.y0 = to30(p.y);
    scalar_mul_task<H>(io);
    p = io.oid ? Affine<F>::identity() : Affine<F>{from30(io.ox), neg ? from30(io.oy).neg() : from30(io.oy)};
    return G16_OK;
}

template <class F, class Fr>
void host_stage(Affine<F>* d, uint64_t count, int half_log, const Fr* tw, int tw_shift, bool scaled, const Fr& scale, bool odd_only) {
    const uint64_t half = (uint64_t)1 << half_log;
    for (uint64_t t = 0; t < count; ++t) {
        const uint64_t i = lag_index(t, half_log), e = (t & (half - 1)) << tw_shift;
        LagHostIO<F> io;
        io.a = d[i];
        io.b = d[i + half];
        lagrange_addsub_task<typename Lazy<F>::host>(io);
        if (scaled) {
            host_twiddle_mul(io.s, scale);
            host_twiddle_mul(io.d, tw[e] * scale);
        } else if (e) {
            host_twiddle_mul(io.d, tw[e]);
        }
        if (!odd_only) d[i] = io.s;
        d[i + half] = io.d;
    }
}
template <class F, class Fr>
void host_stages(Affine<F>* d, int log_n, const Fr* tw, int tw_extra, bool scaled, const Fr& scale) {
    const uint64_t count = ((uint64_t)1 << log_n) >> 1;
    for (int s = 0; s < log_n; ++s) host_stage<F, Fr>(d, count, log_n - 1 - s, tw, s + tw_extra, scaled && s == 0, scale, false);
}
template <class A>
void host_bitrev(const A* in, int log_n, A* out) {
    for (uint64_t i = 0; i < ((uint64_t)1 << log_n); ++i) {
        uint64_t r = 0;
        for (int b = 0; b < log_n; ++b) r |= ((i >> b) & 1) << (log_n - 1 - b);
        out[i] = in[r];
    }
}
template <class F, class Fr>
void host_lagrange_array(const uint64_t* in, int log_n, const Fr* tw, int tw_extra, uint64_t* out) {
    const uint64_t n = (uint64_t)1 << log_n;
    std::vector<Affine<F>> work(n);
    memcpy(work.data(), in, n * sizeof(Affine<F>));
    host_stages<F, Fr>(work.data(), log_n, tw, tw_extra, true, Fr::from_u64(n).inverse());
    host_bitrev(work.data(), log_n, reinterpret_cast<Affine<F>*>(out));
}

}  // namespace

// ---- g16_group_ntt_windowed -----------------------------------------------------------------------------------------------------------
template <class C, int G2>
int group_ntt_windowed_any(const CeremonyEnv* env, const uint64_t* points, int log_n, int inverse, uint64_t* out, g16_lagrange_timings* tm) {
    typedef typename C::Fr Fr;
    typedef Dev<C, G2> D;
    typedef typename D::A A;
    if (log_n < 0 || log_n > C::TWO_ADICITY || log_n > 30) return G16_ERR_DEGREE_TOO_LARGE;
    const uint64_t n = (uint64_t)1 << log_n;
    const Fr w = root_of<C>(log_n);
    const std::vector<Fr> tw = power_table(inverse ? w.inverse() : w, n / 2);
    const Fr scale = Fr::from_u64(n).inverse();
    if (!env) {
        std::vector<A> work(n);
        memcpy(work.data(), points, n * sizeof(A));
        host_stages<typename D::F, Fr>(work.data(), log_n, tw.data(), 0, inverse != 0, scale);
        host_bitrev(work.data(), log_n, reinterpret_cast<A*>(out));
        return G16_OK;
    }
    const uint64_t chunk = std::min(std::max<uint64_t>(n / 2, 1), lagrange_chunk());
    Fr* d_tw = nullptr;
    A *work = nullptr, *rev = nullptr;
    uint32_t* park = nullptr;
    Timers timer;
    StreamWait wait{env->st};   // tw is read by the upload
    G16_TRY(upload(*env, tw.data(), tw.size(), &d_tw));
    G16_TRY(env->arena->alloc_n(n, &work));
    G16_TRY(env->arena->alloc_n(n, &rev));
    G16_TRY(env->arena->alloc_n(D::park_words(chunk), &park));
    EventTimer* t = timer.add();
    G16_TRY(t->start(env->st));
    G16_HIP_TRY(hipMemcpyAsync(work, points, n * sizeof(A), hipMemcpyHostToDevice, env->st));
    G16_TRY(D::stages(env->st, work, log_n, d_tw, 0, inverse != 0, scale, chunk, park));
    G16_TRY(D::bitrev(env->st, work, log_n, rev));
    G16_HIP_TRY(hipMemcpyAsync(out, rev, n * sizeof(A), hipMemcpyDeviceToHost, env->st));
    G16_TRY(t->stop(env->st));
    G16_HIP_TRY(hipStreamSynchronize(env->st));
    (G2 ? tm->u_g2_ms : tm->u_g1_ms) = timer.total();
    return G16_OK;
}

// ---- g16_srs_lagrange -----------------------------------------------------------------------------------------------------------------
template <class C>
int srs_lagrange_any(const CeremonyEnv* env, const g16_srs_view* srs, int log_n, int qap, g16_lagrange_srs_view* out, g16_lagrange_timings* tm) {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef Affine<Fq> A1;
    typedef Affine<Fq2> A2;
    const bool circom = qap == G16_QAP_CIRCOM;
    if (log_n < 0 || log_n > 30 || log_n + (circom ? 1 : 0) > C::TWO_ADICITY) return G16_ERR_DEGREE_TOO_LARGE;
    const uint64_t n = (uint64_t)1 << log_n, n_tau = 2 * n - 1, n_h = circom ? n : n - 1;
    const SrsArray need[] = {{"tau_g1", srs->n_tau_g1, n_tau}, {"tau_g2", srs->n_tau_g2, n}, {"alpha_tau_g1 / beta_tau_g1 (one count)", srs->n_alpha_beta, n}};
    G16_TRY(srs_lengths(need, "SRS too short: %s holds %llu points, %llu are needed for a domain of %llu", n));
    // inverse twiddles: w^-e, e < n / 2 -- or rho^-e, e < n, of the 2n-point domain (w = rho^2: the n-point stages read every other one)
    const Fr root = root_of<C>(log_n + (circom ? 1 : 0));
    const std::vector<Fr> tw = power_table(root.inverse(), circom ? n : n / 2);
    const int tw_extra = circom ? 1 : 0;
    const Fr scale2 = Fr::from_u64(2 * n).inverse();
    if (!env) {
        host_lagrange_array<Fq, Fr>(srs->tau_g1, log_n, tw.data(), tw_extra, out->u_g1);
        host_lagrange_array<Fq, Fr>(srs->alpha_tau_g1, log_n, tw.data(), tw_extra, out->alpha_u_g1);
        host_lagrange_array<Fq, Fr>(srs->beta_tau_g1, log_n, tw.data(), tw_extra, out->beta_u_g1);
        host_lagrange_array<Fq2, Fr>(srs->tau_g2, log_n, tw.data(), tw_extra, out->u_g2);
        std::vector<A1> work(2 * n, A1::identity());
        memcpy(work.data(), srs->tau_g1, n_tau * sizeof(A1));
        A1* h = reinterpret_cast<A1*>(out->h_g1);
        if (!circom) {
            for (uint64_t i = 0; i < n_h; ++i) {   // tau_g1[i + n] - tau_g1[i]
                LagHostIO<Fq> io;
                io.a = work[i + n];
                io.b = work[i];
                lagrange_addsub_task<typename Lazy<Fq>::host>(io);
                h[i] = io.d;
            }
        } else {
            host_stage<Fq, Fr>(work.data(), n, log_n, tw.data(), 0, true, scale2, true);
            host_stages<Fq, Fr>(work.data() + n, log_n, tw.data(), 1, false, Fr::one());
            host_bitrev(work.data() + n, log_n, h);
        }
    } else {
        typedef Dev<C, 0> D1;
        typedef Dev<C, 1> D2;
        const uint64_t chunk = std::min(n, lagrange_chunk());
        Fr* d_tw = nullptr;
        A1 *work1 = nullptr, *rev1 = nullptr;
        A2 *work2 = nullptr, *rev2 = nullptr;
        uint32_t* park = nullptr;
        EventTimer et[5];
        auto body = [&]() -> int {
            G16_TRY(upload(*env, tw.data(), tw.size(), &d_tw));
            G16_TRY(env->arena->alloc_n(2 * n, &work1));
            G16_TRY(env->arena->alloc_n(n, &rev1));
            G16_TRY(env->arena->alloc_n(n, &work2));
            G16_TRY(env->arena->alloc_n(n, &rev2));
            G16_TRY(env->arena->alloc_n(std::max(D1::park_words(chunk), D2::park_words(chunk)), &park));
            G16_TRY(D1::lagrange_array(*env, srs->tau_g1, log_n, d_tw, tw_extra, work1, rev1, chunk, park, out->u_g1, et[0]));
            G16_TRY(D1::lagrange_array(*env, srs->alpha_tau_g1, log_n, d_tw, tw_extra, work1, rev1, chunk, park, out->alpha_u_g1, et[1]));
            G16_TRY(D1::lagrange_array(*env, srs->beta_tau_g1, log_n, d_tw, tw_extra, work1, rev1, chunk, park, out->beta_u_g1, et[2]));
            G16_TRY(D2::lagrange_array(*env, srs->tau_g2, log_n, d_tw, tw_extra, work2, rev2, chunk, park, out->u_g2, et[3]));
            // the h basis
            G16_TRY(et[4].start(env->st));
            G16_HIP_TRY(hipMemcpyAsync(work1, srs->tau_g1, n_tau * sizeof(A1), hipMemcpyHostToDevice, env->st));
            if (!circom) {
                for (uint64_t t0 = 0; t0 < n_h; t0 += chunk)   // tau_g1[i + n] - tau_g1[i]
                    G16_TRY(D1::addsub(env->st, work1 + n, work1, nullptr, rev1, t0, std::min(chunk, n_h - t0), LAG_LINEAR));
            } else {
                G16_HIP_TRY(hipMemsetAsync(work1 + n_tau, 0, sizeof(A1), env->st));   // the identity pads 2n - 1 powers to 2n
                G16_TRY(D1::stage(env->st, work1, n, log_n, d_tw, 0, true, scale2, true, chunk, park));
                G16_TRY(D1::stages(env->st, work1 + n, log_n, d_tw, 1, false, Fr::one(), chunk, park));
                G16_TRY(D1::bitrev(env->st, work1 + n, log_n, rev1));
            }
            if (n_h) G16_HIP_TRY(hipMemcpyAsync(out->h_g1, rev1, n_h * sizeof(A1), hipMemcpyDeviceToHost, env->st));
            G16_TRY(et[4].stop(env->st));
            return G16_OK;
        };
        const int rc = body();
        const hipError_t se = hipStreamSynchronize(env->st);   // tw goes out of scope; launches into the arena must not outlive the call
        if (rc == G16_OK && se == hipSuccess) {
            tm->u_g1_ms = et[0].ms(); tm->alpha_u_g1_ms = et[1].ms(); tm->beta_u_g1_ms = et[2].ms(); tm->u_g2_ms = et[3].ms(); tm->h_ms = et[4].ms();
        }
        for (auto& t : et) t.destroy();
        G16_TRY(rc);
        G16_HIP_TRY(se);
    }
    memcpy(out->tau_g1_0, srs->tau_g1, sizeof(A1));
    memcpy(out->alpha_g1_0, srs->alpha_tau_g1, sizeof(A1));
    memcpy(out->beta_g1_0, srs->beta_tau_g1, sizeof(A1));
    memcpy(out->tau_g2_0, srs->tau_g2, sizeof(A2));
    memcpy(out->beta_g2, srs->beta_g2, sizeof(A2));
    out->log_n = log_n;
    out->qap = qap;
    return G16_OK;
}

// ---- g16_generate_parameters_lagrange -------------------------------------------------------------------------------------------------
template <class C>
int generate_lagrange_any(const CeremonyEnv* env, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, const g16_lagrange_srs_view* lag,
                          const g16_params_view* out, g16_lagrange_timings* tm) {
    typedef Affine<typename C::Fq> A1;
    typedef Affine<typename C::Fq2> A2;
    if (lag->qap != G16_QAP_LIBSNARK && lag->qap != G16_QAP_CIRCOM)
        return refuse(G16_ERR_BAD_ARG, "Lagrange SRS: qap %s%llu is neither G16_QAP_LIBSNARK nor G16_QAP_CIRCOM", (unsigned long long)lag->qap, 0, 0);
    int log_n = 0;
    G16_TRY(srs_domain_log<C>(ni, nc, nv, lag->qap, &log_n));
    if (log_n != lag->log_n)
        return refuse(G16_ERR_BAD_LENGTH, "Lagrange SRS: %sprepared for a domain of 2^%llu points, the circuit's domain is 2^%llu",
                      (unsigned long long)lag->log_n, (unsigned long long)log_n, 0);
    const uint64_t n = (uint64_t)1 << log_n, n_h = lag->qap == G16_QAP_CIRCOM ? n : n - 1;
    g16_srs_view fixed = {};   // index 0 of each array is all the tail reads
    fixed.tau_g1 = lag->tau_g1_0; fixed.alpha_tau_g1 = lag->alpha_g1_0; fixed.beta_tau_g1 = lag->beta_g1_0; fixed.tau_g2 = lag->tau_g2_0;
    fixed.beta_g2 = lag->beta_g2;
    fixed.n_tau_g1 = fixed.n_tau_g2 = fixed.n_alpha_beta = 1;
    if (!env) {
        G16_TRY(srs_queries_host<C>(abc, ni, nc, nv, lag->u_g1, lag->alpha_u_g1, lag->beta_u_g1, lag->u_g2, &fixed, out));
    } else {
        A1* d_u1 = nullptr;   // u | alpha u | beta u
        A2* d_u2 = nullptr;
        StreamWait wait{env->st};
        G16_TRY(env->arena->alloc_n(3 * n, &d_u1));
        G16_TRY(env->arena->alloc_n(n, &d_u2));
        G16_HIP_TRY(hipMemcpyAsync(d_u1, lag->u_g1, n * sizeof(A1), hipMemcpyHostToDevice, env->st));
        G16_HIP_TRY(hipMemcpyAsync(d_u1 + n, lag->alpha_u_g1, n * sizeof(A1), hipMemcpyHostToDevice, env->st));
        G16_HIP_TRY(hipMemcpyAsync(d_u1 + 2 * n, lag->beta_u_g1, n * sizeof(A1), hipMemcpyHostToDevice, env->st));
        G16_HIP_TRY(hipMemcpyAsync(d_u2, lag->u_g2, n * sizeof(A2), hipMemcpyHostToDevice, env->st));
        G16_TRY(srs_queries_device<C>(env->st, *env->arena, abc, ni, nc, nv, log_n, reinterpret_cast<const uint64_t*>(d_u1),
                                      reinterpret_cast<const uint64_t*>(d_u2), &fixed, out, &tm->products_ms));
    }
    if (n_h) memcpy(out->h_query, lag->h_g1, n_h * sizeof(A1));
    return G16_OK;
}

namespace {
bool lagrange_view_ok(const g16_lagrange_srs_view* v) {
    return v->u_g1 && v->alpha_u_g1 && v->beta_u_g1 && v->u_g2 && v->h_g1 && v->tau_g1_0 && v->alpha_g1_0 && v->beta_g1_0 && v->tau_g2_0 && v->beta_g2;
}
int ntt_args(int g2, const uint64_t* points, const uint64_t* out) {
    if (g2 != 0 && g2 != 1) return G16_ERR_BAD_ARG;
    return (points && out) ? G16_OK : G16_ERR_BAD_ARG;
}
int prepare_args(const g16_srs_view* srs, int qap, const g16_lagrange_srs_view* out) {
    if (!srs || !out || !srs_view_ok(srs)) return G16_ERR_BAD_ARG;
    if (qap != G16_QAP_LIBSNARK && qap != G16_QAP_CIRCOM) return G16_ERR_BAD_ARG;
    return lagrange_view_ok(out) ? G16_OK : G16_ERR_BAD_ARG;
}
int generate_args(const g16_csr_view* abc, uint64_t ni, uint64_t nv, const g16_lagrange_srs_view* lag, const g16_params_view* out) {
    if (!abc || !lag || !out || !lagrange_view_ok(lag)) return G16_ERR_BAD_ARG;
    if (!out->alpha_g1 || !out->beta_g1 || !out->delta_g1 || !out->beta_g2 || !out->delta_g2 || !out->gamma_g2) return G16_ERR_BAD_ARG;
    if (out->flags & G16_PARAMS_DEVICE_PTRS) return G16_ERR_BAD_ARG;
    return (out->gamma_abc_g1 && out->a_query && out->b_g1_query && out->b_g2_query && out->h_query && (out->l_query || nv <= ni)) ? G16_OK
                                                                                                                                 : G16_ERR_BAD_ARG;
}
}  // namespace

}  // namespace g16

extern "C" {

int g16_group_ntt_windowed(g16_ctx* ctx, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out) {
    if (!ctx) return G16_ERR_BAD_ARG;
    G16_TRY(ntt_args(g2, points, out));
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    g16_lagrange_timings* tm = Stages::of(lagrange_stage_ms(ctx));
    *tm = g16_lagrange_timings{};
    if (g2) G16_VERIFY_DISPATCH(curve, (group_ntt_windowed_any<CC, 1>(&env, points, log_n, inverse, out, tm)));
    G16_VERIFY_DISPATCH(curve, (group_ntt_windowed_any<CC, 0>(&env, points, log_n, inverse, out, tm)));
}

int g16_host_group_ntt_windowed(int curve, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out) {
    G16_TRY(ntt_args(g2, points, out));
    if (g2) G16_VERIFY_DISPATCH(curve, (group_ntt_windowed_any<CC, 1>(nullptr, points, log_n, inverse, out, nullptr)));
    G16_VERIFY_DISPATCH(curve, (group_ntt_windowed_any<CC, 0>(nullptr, points, log_n, inverse, out, nullptr)));
}

int g16_srs_lagrange(g16_ctx* ctx, const g16_srs_view* srs, int log_n, int qap, g16_lagrange_srs_view* out) {
    if (!ctx) return G16_ERR_BAD_ARG;
    G16_TRY(prepare_args(srs, qap, out));
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    g16_lagrange_timings* tm = Stages::of(lagrange_stage_ms(ctx));
    *tm = g16_lagrange_timings{};
    G16_VERIFY_DISPATCH(curve, (srs_lagrange_any<CC>(&env, srs, log_n, qap, out, tm)));
}

int g16_host_srs_lagrange(int curve, const g16_srs_view* srs, int log_n, int qap, g16_lagrange_srs_view* out) {
    G16_TRY(prepare_args(srs, qap, out));
    G16_VERIFY_DISPATCH(curve, (srs_lagrange_any<CC>(nullptr, srs, log_n, qap, out, nullptr)));
}

int g16_generate_parameters_lagrange(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables,
                                     const g16_lagrange_srs_view* lagrange, const g16_params_view* out) {
    if (!ctx) return G16_ERR_BAD_ARG;
    G16_TRY(generate_args(abc, num_inputs, num_variables, lagrange, out));
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    g16_lagrange_timings* tm = Stages::of(lagrange_stage_ms(ctx));
    tm->products_ms = 0;   // the preparation's times stay: the two calls are reported side by side
    G16_VERIFY_DISPATCH(curve, (generate_lagrange_any<CC>(&env, abc, num_inputs, num_constraints, num_variables, lagrange, out, tm)));
}

int g16_host_generate_parameters_lagrange(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                          uint64_t num_variables, const g16_lagrange_srs_view* lagrange, const g16_params_view* out) {
    G16_TRY(generate_args(abc, num_inputs, num_variables, lagrange, out));
    G16_VERIFY_DISPATCH(curve, (generate_lagrange_any<CC>(nullptr, abc, num_inputs, num_constraints, num_variables, lagrange, out, nullptr)));
}

int g16_lagrange_get_timings(g16_ctx* ctx, g16_lagrange_timings* out) {
    return Stages::get(lagrange_stage_ms(ctx), out);
}

}  // extern "C"
