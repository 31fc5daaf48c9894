// Trapdoor-free setup: a circuit's proving key from a phase-1 SRS (tau^i G1, tau^i G2, alpha tau^i G1, beta tau^i G1, beta G2), and a
// delta contribution on top of it.  Nobody holds tau, alpha or beta here, so every step of setup.hip that multiplies a SCALAR by the
// generator becomes the same linear map applied to POINTS:
//
//   1. Lagrange-basis points.  L_i(tau) = n^-1 sum_k tau^k w^(-ik), so [L_i(tau)] G is the inverse n-point transform OVER THE GROUP of the
//      first n SRS powers -- four times: tau_g1, alpha_tau_g1, beta_tau_g1 (G1), tau_g2 (G2).  This stands in for
//      evaluate_all_lagrange_coefficients + the fixed-base multiplications (r1cs_to_qap.rs:120-170, generator.rs:129-183).
//        radix-2 Gentleman-Sande over XYZZ<F>, one launch per stage, one lane per butterfly:  a' = a + b,  b' = w^-(k << s) (a - b).
//        A butterfly costs one scalar multiplication by a full-size Fr twiddle (~255 doublings + ~127 additions, thousands of field
//        products) against 2 x 4 coordinates of traffic, so the stages are compute-bound by three orders of magnitude and fusing them
//        through LDS would buy nothing.  Twiddle 1 (k = 0: all of the last stage, half of the one before; -1 never occurs below n / 2)
//        takes no multiplication.  n^-1 rides on stage 0, where it costs n / 2 + 1 extra multiplications (b's twiddle becomes n^-1 w^-k,
//        a' is multiplied by n^-1) instead of n at the end.  Values stay XYZZ between stages; one inversion per point at the end, fused
//        with the bit reversal (srs_normalize_kernel).
//   2. Queries.  Setup::qap_evaluations with scalars replaced by points: out[j] = sum_i M[i][j] u[i] -- a sparse product over COLUMNS.
//      The host transposes (counting sort, O(nnz)) and cuts every column into segments of at most SRS_SEGMENT_LEN entries; a lane walks
//      one segment (srs_colsum_kernel), further levels fold SRS_SEGMENT_LEN segment sums at a time (srs_colfold_kernel) until every
//      column has one, and srs_colfinish_kernel normalises.  So no lane ever walks more than SRS_SEGMENT_LEN terms, whatever the
//      constant-one column of a real circuit holds.  The coefficients stay on the device in Montgomery form, read through the
//      transposed index: 0 contributes nothing, 1 and r - 1 take no multiplication, the rest multiply over the bits of min(v, r - v).
//   3. h_query (r1cs_to_qap.rs:236-246 with delta = 1).  Libsnark: tau_g1[i + n] - tau_g1[i].  Circom: the odd outputs of the inverse
//      2n-point transform of tau_g1[0 .. 2n-1) | O.  Stage 0 of that transform already separates them -- X[2m+1] is the n-point
//      transform of (2n)^-1 rho^-k (x[k] - x[k+n]) -- so it runs for the b' half alone and the n-point stages follow on that half.
//   4. A delta contribution: delta_g1, delta_g2 <- delta (.) (two points: host), l_query and h_query <- delta^-1 (.)
//      (srs_scale_kernel: every lane shares the scalar, so its bits steer the whole wave the same way).
//
// The derivation is cut where the Lagrange points and the h points are complete: plan_queries (host: transposition, segment plans) and
// run_queries_device / queries_host are step 2 as pieces of their own, so that libg16_lagrange.so (lagrange.hip) can
// run them on Lagrange points that were made once and kept (srs_queries_device / srs_queries_host in srs_setup.hpp).
//
// Affine Montgomery coordinates are canonical: the key equals generate_parameters_with_qap(alpha, beta, 1, delta, t = tau) bit for bit
// however the sums were grouped.  The *_host functions run the same butterflies and the same sums in plain host C++ (no GPU).
#include "srs_setup.hpp"
#include <algorithm>
#include <thread>

namespace g16 {

enum { SRS_BF_SCALE = 1, SRS_BF_ODD_ONLY = 2 };

G16_HD uint64_t srs_bitrev(uint64_t i, int bits) {
    uint64_t r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

// k * p over the bits of min(k, r - k)
template <class F, class Fr>
G16_HD XYZZ<F> srs_scalar_mul(const XYZZ<F>& p, const Fr& k) {
    uint32_t c[Fr::N], d[Fr::N];
    k.to_canonical(c);
    k.neg().to_canonical(d);
    bool neg = false;   // d < c
    for (int i = Fr::N - 1; i >= 0; --i)
        if (c[i] != d[i]) { neg = d[i] < c[i]; break; }
    if (neg) for (int i = 0; i < Fr::N; ++i) c[i] = d[i];
    int bits = 0;
    for (int i = Fr::N - 1; i >= 0; --i)
        if (c[i]) {
            bits = 32 * i + 32;
            while (!((c[i] >> ((bits - 1) & 31)) & 1)) --bits;
            break;
        }
    const XYZZ<F> r = p.mul_bits(c, bits);
    return neg ? r.neg() : r;
}

// butterfly t of a Gentleman-Sande stage over blocks of 2^(half_log + 1): the complete addition throughout (P + P, P - P, O)
template <class F, class Fr>
G16_HD void srs_butterfly(XYZZ<F>* data, const Fr* tw, const Fr& scale, uint64_t t, int half_log, int tw_shift, int flags) {
    const uint64_t half = (uint64_t)1 << half_log, k = t & (half - 1), i = ((t >> half_log) << (half_log + 1)) + k;
    XYZZ<F> a = data[i];
    const XYZZ<F> b = data[i + half];
    XYZZ<F> d = a;
    d.add(b.neg());
    if (!(flags & SRS_BF_ODD_ONLY)) {
        a.add(b);
        if (flags & SRS_BF_SCALE) a = srs_scalar_mul(a, scale);
        data[i] = a;
    }
    const uint64_t e = k << tw_shift;
    if (flags & SRS_BF_SCALE) d = srs_scalar_mul(d, e ? tw[e] * scale : scale);
    else if (e) d = srs_scalar_mul(d, tw[e]);
    data[i + half] = d;
}

template <class F, class Fr>
G16_HD XYZZ<F> srs_term(const Affine<F>& p, const Fr& v) {
    if (v == Fr::one()) return XYZZ<F>::from_affine(p);
    if (v == Fr::one().neg()) return XYZZ<F>::from_affine(p.neg());
    return srs_scalar_mul(XYZZ<F>::from_affine(p), v);
}

// a scalar shared by a whole launch: canonical words and its bit length
struct SrsBits {
    uint32_t w[8];
    int bits;
};

// ---- kernels: one lane per element, 64-lane groups (every lane runs whole group operations out of registers / scratch, no LDS) ----

// out[i] = in[i] for i < n_in, the identity above (the Circom h transform pads 2n - 1 powers to 2n)
template <class F>
__global__ __launch_bounds__(64) void srs_lift_kernel(const Affine<F>* __restrict__ in, uint64_t n_in, XYZZ<F>* __restrict__ out, uint64_t n_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_out) return;
    out[i] = i < n_in ? XYZZ<F>::from_affine(in[i]) : XYZZ<F>::identity();
}

// one stage, in place: lane t owns data[i] and data[i + half] alone.  tw holds count << tw_shift entries at least (the caller's table
// covers half the domain the stage belongs to)
template <class F, class Fr>
__global__ __launch_bounds__(64) void srs_butterfly_kernel(XYZZ<F>* data, const Fr* __restrict__ tw, Fr scale, uint64_t count, int half_log,
                                                           int tw_shift, int flags) {
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= count) return;
    srs_butterfly<F, Fr>(data, tw, scale, t, half_log, tw_shift, flags);
}

// out[i] = in[bitrev(i)] as an affine point: the one inversion per point of a transform
template <class F>
__global__ __launch_bounds__(64) void srs_normalize_kernel(const XYZZ<F>* __restrict__ in, int bits, Affine<F>* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    out[i] = in[srs_bitrev(i, bits)].to_affine();
}

// partial[t] = sum over the entries [task_start[t], task_start[t + 1]) -- at most SRS_SEGMENT_LEN of them, all of one column -- of
// vals[ent_val[e]] * pts[ent_pt[e]]
template <class F, class Fr>
__global__ __launch_bounds__(64) void srs_colsum_kernel(const Affine<F>* __restrict__ pts, const Fr* __restrict__ vals,
                                                        const uint32_t* __restrict__ ent_pt, const uint32_t* __restrict__ ent_val,
                                                        const uint32_t* __restrict__ task_start, uint32_t n_tasks, XYZZ<F>* __restrict__ partial) {
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= n_tasks) return;
    XYZZ<F> acc = XYZZ<F>::identity();
    const uint32_t hi = task_start[t + 1];
    for (uint32_t e = task_start[t]; e < hi; ++e) {
        const Fr v = vals[ent_val[e]];
        if (v.is_zero()) continue;
        acc.add(srs_term<F, Fr>(pts[ent_pt[e]], v));
    }
    partial[t] = acc;
}

// the next level: out[t] = sum of in[task_start[t] .. task_start[t + 1]), at most SRS_SEGMENT_LEN segment sums of one column
template <class F>
__global__ __launch_bounds__(64) void srs_colfold_kernel(const XYZZ<F>* __restrict__ in, const uint32_t* __restrict__ task_start, uint32_t n_tasks,
                                                         XYZZ<F>* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= n_tasks) return;
    XYZZ<F> acc = XYZZ<F>::identity();
    const uint32_t hi = task_start[t + 1];
    for (uint32_t e = task_start[t]; e < hi; ++e) acc.add(in[e]);
    out[t] = acc;
}

// column j has one sum (col_ptr[j + 1] == col_ptr[j] + 1) or none: an empty column is the identity (0, 0)
template <class F>
__global__ __launch_bounds__(64) void srs_colfinish_kernel(const XYZZ<F>* __restrict__ partial, const uint32_t* __restrict__ col_ptr, uint64_t n_cols,
                                                           Affine<F>* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n_cols) return;
    const uint32_t lo = col_ptr[j];
    out[j] = col_ptr[j + 1] > lo ? partial[lo].to_affine() : Affine<F>::identity();
}

// out[i] = hi[i] - lo[i]   (Libsnark h_query: tau^i Z(tau) G1)
template <class F>
__global__ __launch_bounds__(64) void srs_diff_kernel(const Affine<F>* __restrict__ hi, const Affine<F>* __restrict__ lo, uint64_t n,
                                                      Affine<F>* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    XYZZ<F> acc = XYZZ<F>::from_affine(hi[i]);
    acc.add_affine(lo[i].neg());
    out[i] = acc.to_affine();
}

// pts[i] <- k * pts[i], one scalar for all lanes: the branch on a bit of k is uniform across the wave
template <class F>
__global__ __launch_bounds__(64) void srs_scale_kernel(Affine<F>* pts, uint64_t n, SrsBits k) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p = pts[i];
    XYZZ<F> acc = XYZZ<F>::identity();
    for (int b = k.bits - 1; b >= 0; --b) {
        acc = acc.dbl();
        if ((k.w[b >> 5] >> (b & 31)) & 1) acc.add_affine(p);
    }
    pts[i] = acc.to_affine();
}

namespace {

inline unsigned srs_blocks(uint64_t n) { return (unsigned)((n + 63) / 64); }

// the host twins' butterflies of one stage are independent: a few threads keep the CPU tier's larger cases in seconds
template <class Fn>
void srs_parallel_for(uint64_t n, Fn fn) {
    const uint64_t nt = std::min<uint64_t>(std::min(8u, std::max(1u, std::thread::hardware_concurrency())), n / 16);
    if (nt <= 1) {
        for (uint64_t t = 0; t < n; ++t) fn(t);
        return;
    }
    std::vector<std::thread> th;
    for (uint64_t k = 0; k < nt; ++k)
        th.emplace_back([=]() { for (uint64_t t = n * k / nt; t < n * (k + 1) / nt; ++t) fn(t); });
    for (auto& x : th) x.join();
}

// the transposed matrices of one query: entry e of column j reads point ent_pt[e] and coefficient ent_val[e]
struct SrsCsc {
    std::vector<uint32_t> col_ptr, ent_pt, ent_val;
};
// the segment plan over a CSC: levels[0] cuts the entries, levels[k] the sums of level k - 1; last_ptr: each column's one sum (or none)
struct SrsPlan {
    std::vector<std::vector<uint32_t>> levels;
    std::vector<uint32_t> last_ptr;
};

template <class C>
struct Srs {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;

    static Fr root_of(int log_n) {
        Fr w = C::two_adic_root();
        for (int k = log_n; k < C::TWO_ADICITY; ++k) w = w.sqr();
        return w;
    }
    // tw[e] = base^e, e < count
    static std::vector<Fr> power_table(const Fr& base, uint64_t count) {
        std::vector<Fr> tw(count ? count : 1);
        Fr p = Fr::one();
        for (auto& x : tw) { x = p; p = p * base; }
        return tw;
    }

    // ---- transposition and the segment plan (host, O(nnz)) ----------------------------------------------------------------------
    // mats[m] over the points at pt_off[m] and the coefficients at val_off[m] (their positions in the device copies); `extra`:
    // column j < ni also gets the point extra_pt + j with the coefficient at one_val (the instance rows of r1cs_to_qap.rs:150-155)
    static int transpose(const g16_csr_view* const* mats, const uint64_t* pt_off, const uint64_t* val_off, int n_mats, uint64_t nc, uint64_t nv,
                         bool extra, uint64_t ni, uint64_t extra_pt, uint64_t one_val, SrsCsc* out) {
        std::vector<uint64_t> cnt(nv + 1, 0);
        for (int m = 0; m < n_mats; ++m) {
            const g16_csr_view& v = *mats[m];
            for (uint64_t k = v.row_ptr[0]; k < v.row_ptr[nc]; ++k) {
                if (v.col[k] >= nv) return G16_ERR_BAD_LENGTH;
                ++cnt[v.col[k] + 1];
            }
        }
        if (extra) for (uint64_t j = 0; j < ni; ++j) ++cnt[j + 1];
        for (uint64_t j = 0; j < nv; ++j) cnt[j + 1] += cnt[j];
        if (cnt[nv] >= ((uint64_t)1 << 32) - 1) return G16_ERR_BAD_LENGTH;   // entries are counted in 32 bits on the device
        out->col_ptr.assign(cnt.begin(), cnt.end());
        out->ent_pt.resize(cnt[nv]);
        out->ent_val.resize(cnt[nv]);
        std::vector<uint64_t> pos(cnt.begin(), cnt.end() - 1);
        for (int m = 0; m < n_mats; ++m) {
            const g16_csr_view& v = *mats[m];
            for (uint64_t i = 0; i < nc; ++i)
                for (uint64_t k = v.row_ptr[i]; k < v.row_ptr[i + 1]; ++k) {
                    const uint64_t p = pos[v.col[k]]++;
                    out->ent_pt[p] = (uint32_t)(pt_off[m] + i);
                    out->ent_val[p] = (uint32_t)(val_off[m] + (k - v.row_ptr[0]));
                }
        }
        if (extra)
            for (uint64_t j = 0; j < ni; ++j) {
                const uint64_t p = pos[j]++;
                out->ent_pt[p] = (uint32_t)(extra_pt + j);
                out->ent_val[p] = (uint32_t)one_val;
            }
        return G16_OK;
    }

    static void plan(const std::vector<uint32_t>& col_ptr, SrsPlan* out) {
        const size_t nv = col_ptr.size() - 1;
        std::vector<uint32_t> ptr = col_ptr;
        out->levels.clear();
        for (bool first = true;; first = false) {
            uint32_t longest = 0;
            for (size_t j = 0; j < nv; ++j) longest = std::max(longest, ptr[j + 1] - ptr[j]);
            if (!first && longest <= 1) break;
            std::vector<uint32_t> ts(1, 0), next(nv + 1, 0);
            for (size_t j = 0; j < nv; ++j) {
                for (uint32_t lo = ptr[j]; lo < ptr[j + 1]; lo += SRS_SEGMENT_LEN) ts.push_back(std::min(lo + SRS_SEGMENT_LEN, ptr[j + 1]));
                next[j + 1] = (uint32_t)(ts.size() - 1);
            }
            out->levels.push_back(std::move(ts));
            ptr.swap(next);
        }
        out->last_ptr.swap(ptr);
    }

    template <class T>
    static int upload(const std::vector<T>& v, Arena& arena, hipStream_t st, T** d) {
        G16_TRY(arena.alloc_n(v.size() ? v.size() : 1, d));
        if (!v.empty()) G16_HIP_TRY(hipMemcpyAsync(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
        return G16_OK;
    }

    struct DevPlan {
        uint32_t *ent_pt = nullptr, *ent_val = nullptr, *last_ptr = nullptr;
        std::vector<uint32_t*> levels;
        std::vector<uint32_t> n_tasks;
        uint64_t n_cols = 0;
    };
    static int upload_plan(const SrsCsc& csc, const SrsPlan& pl, Arena& arena, hipStream_t st, DevPlan* d) {
        G16_TRY(upload(csc.ent_pt, arena, st, &d->ent_pt));
        G16_TRY(upload(csc.ent_val, arena, st, &d->ent_val));
        G16_TRY(upload(pl.last_ptr, arena, st, &d->last_ptr));
        for (const auto& ts : pl.levels) {
            uint32_t* p = nullptr;
            G16_TRY(upload(ts, arena, st, &p));
            d->levels.push_back(p);
            d->n_tasks.push_back((uint32_t)(ts.size() - 1));
        }
        d->n_cols = pl.last_ptr.size() - 1;
        return G16_OK;
    }

    // d_out[j] = sum over column j; buf_a / buf_b: n_tasks[0] and n_tasks[1] (if any) sums of scratch
    template <class F>
    static int col_sums(const DevPlan& d, const Affine<F>* d_pts, const Fr* d_vals, XYZZ<F>* buf_a, XYZZ<F>* buf_b, Affine<F>* d_out, hipStream_t st) {
        if (d.n_tasks[0]) {
            hipLaunchKernelGGL((srs_colsum_kernel<F, Fr>), dim3(srs_blocks(d.n_tasks[0])), dim3(64), 0, st, d_pts, d_vals, d.ent_pt, d.ent_val,
                               d.levels[0], d.n_tasks[0], buf_a);
            G16_LAUNCH_CHECK();
        }
        XYZZ<F>*src = buf_a, *dst = buf_b;
        for (size_t k = 1; k < d.levels.size(); ++k) {
            hipLaunchKernelGGL((srs_colfold_kernel<F>), dim3(srs_blocks(d.n_tasks[k])), dim3(64), 0, st, src, d.levels[k], d.n_tasks[k], dst);
            G16_LAUNCH_CHECK();
            std::swap(src, dst);
        }
        hipLaunchKernelGGL((srs_colfinish_kernel<F>), dim3(srs_blocks(d.n_cols)), dim3(64), 0, st, src, d.last_ptr, d.n_cols, d_out);
        G16_LAUNCH_CHECK();
        return G16_OK;
    }

    // ---- transforms ------------------------------------------------------------------------------------------------------------
    // the stages of a 2^log_n-point transform over d (in place, natural -> bit-reversed); tw[e << tw_extra] is the transform's root^e;
    // scaled: stage 0 also multiplies everything by `scale`
    template <class F>
    static int stages_device(XYZZ<F>* d, int log_n, const Fr* d_tw, int tw_extra, bool scaled, const Fr& scale, hipStream_t st) {
        const uint64_t count = ((uint64_t)1 << log_n) >> 1;
        for (int s = 0; s < log_n; ++s) {
            hipLaunchKernelGGL((srs_butterfly_kernel<F, Fr>), dim3(srs_blocks(count)), dim3(64), 0, st, d, d_tw, scale, count, log_n - 1 - s,
                               s + tw_extra, (scaled && s == 0) ? (int)SRS_BF_SCALE : 0);
            G16_LAUNCH_CHECK();
        }
        return G16_OK;
    }
    template <class F>
    static void stages_host(XYZZ<F>* d, int log_n, const Fr* tw, int tw_extra, bool scaled, const Fr& scale) {
        const uint64_t count = ((uint64_t)1 << log_n) >> 1;
        for (int s = 0; s < log_n; ++s)
            srs_parallel_for(count, [=](uint64_t t) {
                srs_butterfly<F, Fr>(d, tw, scale, t, log_n - 1 - s, s + tw_extra, (scaled && s == 0) ? (int)SRS_BF_SCALE : 0);
            });
    }
    // d_out (affine, natural order) = the inverse n-point transform of d_in[0 .. n), n^-1 included; work: n XYZZ of scratch
    template <class F>
    static int lagrange_device(const Affine<F>* d_in, int log_n, const Fr* d_tw, int tw_extra, XYZZ<F>* work, Affine<F>* d_out, hipStream_t st) {
        const uint64_t n = (uint64_t)1 << log_n;
        hipLaunchKernelGGL((srs_lift_kernel<F>), dim3(srs_blocks(n)), dim3(64), 0, st, d_in, n, work, n);
        G16_LAUNCH_CHECK();
        G16_TRY(stages_device<F>(work, log_n, d_tw, tw_extra, true, Fr::from_u64(n).inverse(), st));
        hipLaunchKernelGGL((srs_normalize_kernel<F>), dim3(srs_blocks(n)), dim3(64), 0, st, work, log_n, d_out, n);
        G16_LAUNCH_CHECK();
        return G16_OK;
    }
    template <class F>
    static void lagrange_host(const Affine<F>* in, int log_n, const Fr* tw, int tw_extra, Affine<F>* out) {
        const uint64_t n = (uint64_t)1 << log_n;
        std::vector<XYZZ<F>> work(n);
        for (uint64_t i = 0; i < n; ++i) work[i] = XYZZ<F>::from_affine(in[i]);
        stages_host<F>(work.data(), log_n, tw, tw_extra, true, Fr::from_u64(n).inverse());
        for (uint64_t i = 0; i < n; ++i) out[i] = work[srs_bitrev(i, log_n)].to_affine();
    }

    // ---- g16_group_ntt -----------------------------------------------------------------------------------------------------------
    template <class F>
    static int group_ntt_device(hipStream_t st, Arena& arena, const uint64_t* points, int log_n, int inverse, uint64_t* out) {
        const uint64_t n = (uint64_t)1 << log_n;
        const Fr w = root_of(log_n);
        const std::vector<Fr> tw = power_table(inverse ? w.inverse() : w, n / 2);
        arena.reset();
        Fr* d_tw = nullptr;
        Affine<F>* d_pts = nullptr;
        XYZZ<F>* work = nullptr;
        G16_TRY(upload(tw, arena, st, &d_tw));
        G16_TRY(arena.alloc_n(n, &d_pts));
        G16_TRY(arena.alloc_n(n, &work));
        G16_HIP_TRY(hipMemcpyAsync(d_pts, points, n * sizeof(Affine<F>), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((srs_lift_kernel<F>), dim3(srs_blocks(n)), dim3(64), 0, st, d_pts, n, work, n);
        G16_LAUNCH_CHECK();
        G16_TRY(stages_device<F>(work, log_n, d_tw, 0, inverse != 0, Fr::from_u64(n).inverse(), st));
        hipLaunchKernelGGL((srs_normalize_kernel<F>), dim3(srs_blocks(n)), dim3(64), 0, st, work, log_n, d_pts, n);
        G16_LAUNCH_CHECK();
        G16_HIP_TRY(hipMemcpyAsync(out, d_pts, n * sizeof(Affine<F>), hipMemcpyDeviceToHost, st));
        G16_HIP_TRY(hipStreamSynchronize(st));   // tw goes out of scope
        return G16_OK;
    }
    template <class F>
    static int group_ntt_host(const uint64_t* points, int log_n, int inverse, uint64_t* out) {
        const uint64_t n = (uint64_t)1 << log_n;
        const Fr w = root_of(log_n);
        const std::vector<Fr> tw = power_table(inverse ? w.inverse() : w, n / 2);
        const Affine<F>* in = reinterpret_cast<const Affine<F>*>(points);
        std::vector<XYZZ<F>> work(n);
        for (uint64_t i = 0; i < n; ++i) work[i] = XYZZ<F>::from_affine(in[i]);
        stages_host<F>(work.data(), log_n, tw.data(), 0, inverse != 0, Fr::from_u64(n).inverse());
        Affine<F>* o = reinterpret_cast<Affine<F>*>(out);
        for (uint64_t i = 0; i < n; ++i) o[i] = work[srs_bitrev(i, log_n)].to_affine();
        return G16_OK;
    }

    // ---- the key ----------------------------------------------------------------------------------------------------------------
    static int check_matrices(const g16_csr_view abc[3], uint64_t nc) {
        for (int m = 0; m < 3; ++m) {
            if (!abc[m].row_ptr || ((!abc[m].col || !abc[m].val) && abc[m].row_ptr[nc] > abc[m].row_ptr[0])) return G16_ERR_BAD_ARG;
            for (uint64_t i = 0; i < nc; ++i)
                if (abc[m].row_ptr[i] > abc[m].row_ptr[i + 1]) return G16_ERR_BAD_LENGTH;
        }
        return G16_OK;
    }
    static void copy_fixed(const g16_srs_view* srs, const g16_params_view* out) {
        memcpy(out->alpha_g1, srs->alpha_tau_g1, sizeof(Affine<Fq>));   // alpha tau^0 G1
        memcpy(out->beta_g1, srs->beta_tau_g1, sizeof(Affine<Fq>));
        memcpy(out->delta_g1, srs->tau_g1, sizeof(Affine<Fq>));         // delta = 1
        memcpy(out->beta_g2, srs->beta_g2, sizeof(Affine<Fq2>));
        memcpy(out->delta_g2, srs->tau_g2, sizeof(Affine<Fq2>));
        memcpy(out->gamma_g2, srs->tau_g2, sizeof(Affine<Fq2>));        // gamma = 1
    }

    // ---- the tail of the derivation: the queries from complete Lagrange points ------------------------------------------------------
    // (generate_device runs it after its transforms; srs_queries_device below runs it on Lagrange points that were made earlier)
    struct SrsQueries {
        SrsCsc csc[3];   // a_query; b_g1_query and b_g2_query; gamma_abc_g1 | l_query over [u | alpha u | beta u]
        SrsPlan pl[3];
        uint64_t nnz[3], voff[3], one_val;
    };
    // host: the transposition and the segment plans over a domain of n points
    static int plan_queries(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, uint64_t n, SrsQueries* q) {
        if (3 * n + ni >= ((uint64_t)1 << 32)) return G16_ERR_DEGREE_TOO_LARGE;   // point indices are 32 bits wide
        for (int m = 0; m < 3; ++m) q->nnz[m] = abc[m].row_ptr[nc] - abc[m].row_ptr[0];
        q->voff[0] = 0; q->voff[1] = q->nnz[0]; q->voff[2] = q->nnz[0] + q->nnz[1];
        q->one_val = q->nnz[0] + q->nnz[1] + q->nnz[2];
        if (q->one_val >= ((uint64_t)1 << 32) - 1) return G16_ERR_BAD_LENGTH;
        const g16_csr_view* ma[1] = {&abc[0]};
        const g16_csr_view* mb[1] = {&abc[1]};
        const g16_csr_view* mm[3] = {&abc[0], &abc[1], &abc[2]};
        const uint64_t p0[1] = {0}, pm[3] = {2 * n, n, 0};
        G16_TRY(transpose(ma, p0, &q->voff[0], 1, nc, nv, true, ni, nc, q->one_val, &q->csc[0]));
        G16_TRY(transpose(mb, p0, &q->voff[1], 1, nc, nv, false, ni, 0, q->one_val, &q->csc[1]));
        G16_TRY(transpose(mm, pm, q->voff, 3, nc, nv, true, ni, 2 * n + nc, q->one_val, &q->csc[2]));
        for (int k = 0; k < 3; ++k) plan(q->csc[k].col_ptr, &q->pl[k]);
        return G16_OK;
    }
    // device: the coefficients and the plans into the arena (on top of what the caller holds there), the column sums, the copies out.
    // d_u1: u | alpha u | beta u, 3n points; d_u2: n points.  The uploads read q and abc: the caller waits for the stream before
    // either goes away
    static int run_queries_device(hipStream_t st, Arena& arena, const SrsQueries& q, const g16_csr_view abc[3], uint64_t ni, uint64_t nv,
                                  const Affine<Fq>* d_u1, const Affine<Fq2>* d_u2, const g16_params_view* out, EventTimer& tm) {
        typedef Affine<Fq> A1;
        typedef Affine<Fq2> A2;
        Fr* d_vals = nullptr;
        A1* d_q1 = nullptr;
        A2* d_q2 = nullptr;
        G16_TRY(arena.alloc_n(q.one_val + 1, &d_vals));
        for (int m = 0; m < 3; ++m)
            if (q.nnz[m])
                G16_HIP_TRY(hipMemcpyAsync(d_vals + q.voff[m], abc[m].val + 4 * abc[m].row_ptr[0], q.nnz[m] * sizeof(Fr), hipMemcpyHostToDevice, st));
        const Fr one = Fr::one();
        G16_HIP_TRY(hipMemcpyAsync(d_vals + q.one_val, &one, sizeof(Fr), hipMemcpyHostToDevice, st));
        DevPlan dp[3];
        uint64_t t0 = 1, t1 = 1;
        for (int k = 0; k < 3; ++k) {
            G16_TRY(upload_plan(q.csc[k], q.pl[k], arena, st, &dp[k]));
            t0 = std::max<uint64_t>(t0, dp[k].n_tasks[0]);
            if (dp[k].n_tasks.size() > 1) t1 = std::max<uint64_t>(t1, dp[k].n_tasks[1]);
        }
        XYZZ<Fq>*pa1 = nullptr, *pb1 = nullptr;
        XYZZ<Fq2>*pa2 = nullptr, *pb2 = nullptr;
        G16_TRY(arena.alloc_n(t0, &pa1));
        G16_TRY(arena.alloc_n(t1, &pb1));
        G16_TRY(arena.alloc_n(t0, &pa2));
        G16_TRY(arena.alloc_n(t1, &pb2));
        G16_TRY(arena.alloc_n(nv, &d_q1));
        G16_TRY(arena.alloc_n(nv, &d_q2));
        G16_TRY(tm.start(st));
        G16_TRY(col_sums<Fq>(dp[0], d_u1, d_vals, pa1, pb1, d_q1, st));
        G16_HIP_TRY(hipMemcpyAsync(out->a_query, d_q1, nv * sizeof(A1), hipMemcpyDeviceToHost, st));
        G16_TRY(col_sums<Fq>(dp[1], d_u1, d_vals, pa1, pb1, d_q1, st));
        G16_HIP_TRY(hipMemcpyAsync(out->b_g1_query, d_q1, nv * sizeof(A1), hipMemcpyDeviceToHost, st));
        G16_TRY(col_sums<Fq2>(dp[1], d_u2, d_vals, pa2, pb2, d_q2, st));
        G16_HIP_TRY(hipMemcpyAsync(out->b_g2_query, d_q2, nv * sizeof(A2), hipMemcpyDeviceToHost, st));
        G16_TRY(col_sums<Fq>(dp[2], d_u1, d_vals, pa1, pb1, d_q1, st));
        G16_HIP_TRY(hipMemcpyAsync(out->gamma_abc_g1, d_q1, ni * sizeof(A1), hipMemcpyDeviceToHost, st));
        if (nv > ni) G16_HIP_TRY(hipMemcpyAsync(out->l_query, d_q1 + ni, (nv - ni) * sizeof(A1), hipMemcpyDeviceToHost, st));
        G16_TRY(tm.stop(st));
        return G16_OK;
    }
    // the tail as a call of its own: the matrices are checked, d_u1 / d_u2 are the caller's (in `arena`, which is not reset here), the
    // fixed points come from index 0 of `fixed`'s arrays.  Returns after the stream has drained
    static int queries_device(hipStream_t st, Arena& arena, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int log_n,
                              const uint64_t* d_u1, const uint64_t* d_u2, const g16_srs_view* fixed, const g16_params_view* out, double* products_ms) {
        G16_TRY(check_matrices(abc, nc));
        SrsQueries q;
        G16_TRY(plan_queries(abc, ni, nc, nv, (uint64_t)1 << log_n, &q));
        EventTimer tm;
        const int rc = run_queries_device(st, arena, q, abc, ni, nv, reinterpret_cast<const Affine<Fq>*>(d_u1), reinterpret_cast<const Affine<Fq2>*>(d_u2),
                                          out, tm);
        const hipError_t se = hipStreamSynchronize(st);
        if (rc == G16_OK && se == hipSuccess) {
            if (products_ms) *products_ms = tm.ms();
            copy_fixed(fixed, out);
        }
        tm.destroy();
        if (rc != G16_OK) return rc;
        G16_HIP_TRY(se);
        return G16_OK;
    }

    static int generate_device(hipStream_t st, Arena& arena, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap,
                               const g16_srs_view* srs, const g16_params_view* out, double phase_ms[3]) {
        typedef Affine<Fq> A1;
        typedef Affine<Fq2> A2;
        int log_n = 0;
        G16_TRY(srs_domain_log<C>(ni, nc, nv, qap, &log_n));
        G16_TRY(check_matrices(abc, nc));
        const uint64_t n = (uint64_t)1 << log_n;
        const bool circom = qap == G16_QAP_CIRCOM;
        SrsQueries q;   // transposed matrices and their segment plans: before any device work, so that a bad matrix is refused at once
        G16_TRY(plan_queries(abc, ni, nc, nv, n, &q));
        // inverse twiddles: w^-e, e < n / 2 -- or rho^-e, e < n, of the 2n-point domain (w = rho^2: the n-point stages read every other one)
        const Fr root = root_of(log_n + (circom ? 1 : 0));
        const std::vector<Fr> tw = power_table(root.inverse(), circom ? n : n / 2);
        const int tw_extra = circom ? 1 : 0;

        arena.reset();
        EventTimer tm[3];
        auto body = [&]() -> int {
            Fr* d_tw = nullptr;
            A1 *d_tau1 = nullptr, *d_in1 = nullptr, *d_u1 = nullptr;
            A2 *d_tau2 = nullptr, *d_u2 = nullptr;
            XYZZ<Fq>* work1 = nullptr;
            XYZZ<Fq2>* work2 = nullptr;
            const uint64_t n_tau = 2 * n - 1, n_h = circom ? n : n - 1;
            G16_TRY(upload(tw, arena, st, &d_tw));
            G16_TRY(arena.alloc_n(n_tau, &d_tau1));
            G16_TRY(arena.alloc_n(n, &d_in1));
            G16_TRY(arena.alloc_n(n, &d_tau2));
            G16_TRY(arena.alloc_n(3 * n, &d_u1));   // u | alpha u | beta u
            G16_TRY(arena.alloc_n(n, &d_u2));
            G16_TRY(arena.alloc_n(2 * n, &work1));
            G16_TRY(arena.alloc_n(n, &work2));
            G16_HIP_TRY(hipMemcpyAsync(d_tau1, srs->tau_g1, n_tau * sizeof(A1), hipMemcpyHostToDevice, st));
            G16_HIP_TRY(hipMemcpyAsync(d_tau2, srs->tau_g2, n * sizeof(A2), hipMemcpyHostToDevice, st));
            // 1. the Lagrange-basis points
            G16_TRY(tm[0].start(st));
            G16_TRY(lagrange_device<Fq>(d_tau1, log_n, d_tw, tw_extra, work1, d_u1, st));
            G16_HIP_TRY(hipMemcpyAsync(d_in1, srs->alpha_tau_g1, n * sizeof(A1), hipMemcpyHostToDevice, st));
            G16_TRY(lagrange_device<Fq>(d_in1, log_n, d_tw, tw_extra, work1, d_u1 + n, st));
            G16_HIP_TRY(hipMemcpyAsync(d_in1, srs->beta_tau_g1, n * sizeof(A1), hipMemcpyHostToDevice, st));
            G16_TRY(lagrange_device<Fq>(d_in1, log_n, d_tw, tw_extra, work1, d_u1 + 2 * n, st));
            G16_TRY(lagrange_device<Fq2>(d_tau2, log_n, d_tw, tw_extra, work2, d_u2, st));
            G16_TRY(tm[0].stop(st));
            // 3. h_query (before the products: it frees nothing, but it needs work1 and d_in1 as they are)
            G16_TRY(tm[2].start(st));
            A1* d_h = d_in1;   // n_h <= n points
            if (!circom) {
                if (n_h) {
                    hipLaunchKernelGGL((srs_diff_kernel<Fq>), dim3(srs_blocks(n_h)), dim3(64), 0, st, d_tau1 + n, d_tau1, n_h, d_h);
                    G16_LAUNCH_CHECK();
                }
            } else {
                hipLaunchKernelGGL((srs_lift_kernel<Fq>), dim3(srs_blocks(2 * n)), dim3(64), 0, st, d_tau1, n_tau, work1, 2 * n);
                G16_LAUNCH_CHECK();
                hipLaunchKernelGGL((srs_butterfly_kernel<Fq, Fr>), dim3(srs_blocks(n)), dim3(64), 0, st, work1, d_tw, Fr::from_u64(2 * n).inverse(), n,
                                   log_n, 0, (int)(SRS_BF_SCALE | SRS_BF_ODD_ONLY));
                G16_LAUNCH_CHECK();
                G16_TRY(stages_device<Fq>(work1 + n, log_n, d_tw, 1, false, Fr::one(), st));
                hipLaunchKernelGGL((srs_normalize_kernel<Fq>), dim3(srs_blocks(n)), dim3(64), 0, st, work1 + n, log_n, d_h, n);
                G16_LAUNCH_CHECK();
            }
            if (n_h) G16_HIP_TRY(hipMemcpyAsync(out->h_query, d_h, n_h * sizeof(A1), hipMemcpyDeviceToHost, st));
            G16_TRY(tm[2].stop(st));
            // 2. the queries
            G16_TRY(run_queries_device(st, arena, q, abc, ni, nv, d_u1, d_u2, out, tm[1]));
            return G16_OK;
        };
        const int rc = body();
        // the host vectors behind the uploads (and, after an error, launches into the arena) must not outlive this call
        const hipError_t se = hipStreamSynchronize(st);
        if (rc == G16_OK && se == hipSuccess) {
            if (phase_ms) for (int k = 0; k < 3; ++k) phase_ms[k] = tm[k].ms();
            copy_fixed(srs, out);
        }
        for (auto& t : tm) t.destroy();
        if (rc != G16_OK) return rc;
        G16_HIP_TRY(se);
        return G16_OK;
    }

    // out[j] += sum_i M[i][j] pts[i], in the matrix's row order
    template <class F>
    static int accumulate_host(const g16_csr_view& m, uint64_t nc, uint64_t nv, const Affine<F>* pts, std::vector<XYZZ<F>>& acc) {
        const Fr* val = reinterpret_cast<const Fr*>(m.val);
        for (uint64_t i = 0; i < nc; ++i)
            for (uint64_t k = m.row_ptr[i]; k < m.row_ptr[i + 1]; ++k) {
                if (m.col[k] >= nv) return G16_ERR_BAD_LENGTH;
                if (val[k].is_zero()) continue;
                acc[m.col[k]].add(srs_term<F, Fr>(pts[i], val[k]));
            }
        return G16_OK;
    }
    template <class F>
    static void store_host(const std::vector<XYZZ<F>>& acc, uint64_t lo, uint64_t hi, uint64_t* out) {
        Affine<F>* o = reinterpret_cast<Affine<F>*>(out);
        for (uint64_t j = lo; j < hi; ++j) o[j - lo] = acc[j].to_affine();
    }

    // the tail on the host: the queries from complete Lagrange points (n points each), in the matrices' row order
    static int queries_host(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, const Affine<Fq>* u, const Affine<Fq>* au,
                            const Affine<Fq>* bu, const Affine<Fq2>* u2, const g16_params_view* out) {
        {
            std::vector<XYZZ<Fq>> a(nv, XYZZ<Fq>::identity());
            for (uint64_t j = 0; j < ni; ++j) a[j] = XYZZ<Fq>::from_affine(u[nc + j]);
            G16_TRY(accumulate_host<Fq>(abc[0], nc, nv, u, a));
            store_host<Fq>(a, 0, nv, out->a_query);
        }
        {
            std::vector<XYZZ<Fq>> b(nv, XYZZ<Fq>::identity());
            G16_TRY(accumulate_host<Fq>(abc[1], nc, nv, u, b));
            store_host<Fq>(b, 0, nv, out->b_g1_query);
            std::vector<XYZZ<Fq2>> b2(nv, XYZZ<Fq2>::identity());
            G16_TRY(accumulate_host<Fq2>(abc[1], nc, nv, u2, b2));
            store_host<Fq2>(b2, 0, nv, out->b_g2_query);
        }
        {
            std::vector<XYZZ<Fq>> m(nv, XYZZ<Fq>::identity());
            for (uint64_t j = 0; j < ni; ++j) m[j] = XYZZ<Fq>::from_affine(bu[nc + j]);
            G16_TRY(accumulate_host<Fq>(abc[0], nc, nv, bu, m));
            G16_TRY(accumulate_host<Fq>(abc[1], nc, nv, au, m));
            G16_TRY(accumulate_host<Fq>(abc[2], nc, nv, u, m));
            store_host<Fq>(m, 0, ni, out->gamma_abc_g1);
            store_host<Fq>(m, ni, nv, out->l_query);
        }
        return G16_OK;
    }

    static int generate_host(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap, const g16_srs_view* srs,
                             const g16_params_view* out) {
        typedef Affine<Fq> A1;
        typedef Affine<Fq2> A2;
        int log_n = 0;
        G16_TRY(srs_domain_log<C>(ni, nc, nv, qap, &log_n));
        G16_TRY(check_matrices(abc, nc));
        const uint64_t n = (uint64_t)1 << log_n;
        const bool circom = qap == G16_QAP_CIRCOM;
        const Fr root = root_of(log_n + (circom ? 1 : 0));
        const std::vector<Fr> tw = power_table(root.inverse(), circom ? n : n / 2);
        const int tw_extra = circom ? 1 : 0;
        const A1* tau1 = reinterpret_cast<const A1*>(srs->tau_g1);
        std::vector<A1> u(n), au(n), bu(n);
        std::vector<A2> u2(n);
        lagrange_host<Fq>(tau1, log_n, tw.data(), tw_extra, u.data());
        lagrange_host<Fq>(reinterpret_cast<const A1*>(srs->alpha_tau_g1), log_n, tw.data(), tw_extra, au.data());
        lagrange_host<Fq>(reinterpret_cast<const A1*>(srs->beta_tau_g1), log_n, tw.data(), tw_extra, bu.data());
        lagrange_host<Fq2>(reinterpret_cast<const A2*>(srs->tau_g2), log_n, tw.data(), tw_extra, u2.data());
        G16_TRY(queries_host(abc, ni, nc, nv, u.data(), au.data(), bu.data(), u2.data(), out));
        A1* h = reinterpret_cast<A1*>(out->h_query);
        if (!circom) {
            for (uint64_t i = 0; i + 1 < n; ++i) {
                XYZZ<Fq> acc = XYZZ<Fq>::from_affine(tau1[i + n]);
                acc.add_affine(tau1[i].neg());
                h[i] = acc.to_affine();
            }
        } else {
            std::vector<XYZZ<Fq>> work(2 * n, XYZZ<Fq>::identity());
            for (uint64_t i = 0; i < 2 * n - 1; ++i) work[i] = XYZZ<Fq>::from_affine(tau1[i]);
            const Fr scale = Fr::from_u64(2 * n).inverse();
            XYZZ<Fq>* wk = work.data();
            const Fr* twp = tw.data();
            srs_parallel_for(n, [=](uint64_t t) { srs_butterfly<Fq, Fr>(wk, twp, scale, t, log_n, 0, SRS_BF_SCALE | SRS_BF_ODD_ONLY); });
            stages_host<Fq>(work.data() + n, log_n, tw.data(), 1, false, Fr::one());
            for (uint64_t i = 0; i < n; ++i) h[i] = work[n + srs_bitrev(i, log_n)].to_affine();
        }
        copy_fixed(srs, out);
        return G16_OK;
    }

    static SrsBits bits_of(const Fr& k) {
        SrsBits b;
        memset(&b, 0, sizeof(b));
        k.to_canonical(b.w);
        b.bits = 0;
        for (int i = 32 * Fr::N - 1; i >= 0; --i)
            if ((b.w[i >> 5] >> (i & 31)) & 1) { b.bits = i + 1; break; }
        return b;
    }

    static int apply_delta_device(hipStream_t st, Arena& arena, const uint64_t* delta_, const g16_params_view* io, uint64_t n_l, uint64_t n_h,
                                  double* delta_ms) {
        typedef Affine<Fq> A1;
        typedef Affine<Fq2> A2;
        Fr delta;
        memcpy(&delta, delta_, sizeof(Fr));
        if (delta.is_zero()) return G16_ERR_UNEXPECTED_IDENTITY;
        const SrsBits inv = bits_of(delta.inverse());
        arena.reset();
        EventTimer tm;
        auto body = [&]() -> int {
            A1* d = nullptr;
            G16_TRY(arena.alloc_n(n_l + n_h, &d));
            if (n_l) G16_HIP_TRY(hipMemcpyAsync(d, io->l_query, n_l * sizeof(A1), hipMemcpyHostToDevice, st));
            if (n_h) G16_HIP_TRY(hipMemcpyAsync(d + n_l, io->h_query, n_h * sizeof(A1), hipMemcpyHostToDevice, st));
            G16_TRY(tm.start(st));
            if (n_l + n_h) {
                hipLaunchKernelGGL((srs_scale_kernel<Fq>), dim3(srs_blocks(n_l + n_h)), dim3(64), 0, st, d, n_l + n_h, inv);
                G16_LAUNCH_CHECK();
            }
            G16_TRY(tm.stop(st));
            if (n_l) G16_HIP_TRY(hipMemcpyAsync(io->l_query, d, n_l * sizeof(A1), hipMemcpyDeviceToHost, st));
            if (n_h) G16_HIP_TRY(hipMemcpyAsync(io->h_query, d + n_l, n_h * sizeof(A1), hipMemcpyDeviceToHost, st));
            return G16_OK;
        };
        const int rc = body();
        const hipError_t se = hipStreamSynchronize(st);
        if (rc == G16_OK && se == hipSuccess && delta_ms) *delta_ms = tm.ms();
        tm.destroy();
        if (rc != G16_OK) return rc;
        G16_HIP_TRY(se);
        // the two single points: host
        A1 d1;
        A2 d2;
        memcpy(&d1, io->delta_g1, sizeof(d1));
        memcpy(&d2, io->delta_g2, sizeof(d2));
        d1 = srs_scalar_mul(XYZZ<Fq>::from_affine(d1), delta).to_affine();
        d2 = srs_scalar_mul(XYZZ<Fq2>::from_affine(d2), delta).to_affine();
        memcpy(io->delta_g1, &d1, sizeof(d1));
        memcpy(io->delta_g2, &d2, sizeof(d2));
        return G16_OK;
    }
};

}  // namespace

template <class C>
int srs_domain_log(uint64_t ni, uint64_t nc, uint64_t nv, int qap, int* log_n_out) {
    if (qap != G16_QAP_LIBSNARK && qap != G16_QAP_CIRCOM) return G16_ERR_BAD_ARG;
    if (ni == 0 || nv < ni) return G16_ERR_BAD_LENGTH;
    const uint64_t need = nc + ni;
    int log_n = 0;
    while (((uint64_t)1 << log_n) < need) {
        ++log_n;
        if (log_n > 40) return G16_ERR_DEGREE_TOO_LARGE;
    }
    if (log_n > C::TWO_ADICITY || log_n > 30) return G16_ERR_DEGREE_TOO_LARGE;
    if (qap == G16_QAP_CIRCOM && log_n + 1 > C::TWO_ADICITY) return G16_ERR_DEGREE_TOO_LARGE;   // D::new(2n) fails
    *log_n_out = log_n;
    return G16_OK;
}

template <class C>
int srs_group_ntt_device(hipStream_t st, Arena& arena, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out) {
    if (log_n < 0 || log_n > C::TWO_ADICITY || log_n > 30) return G16_ERR_DEGREE_TOO_LARGE;
    if (!g2) return Srs<C>::template group_ntt_device<typename C::Fq>(st, arena, points, log_n, inverse, out);
    return Srs<C>::template group_ntt_device<typename C::Fq2>(st, arena, points, log_n, inverse, out);
}
template <class C>
int srs_group_ntt_host(int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out) {
    if (log_n < 0 || log_n > C::TWO_ADICITY || log_n > 30) return G16_ERR_DEGREE_TOO_LARGE;
    if (!g2) return Srs<C>::template group_ntt_host<typename C::Fq>(points, log_n, inverse, out);
    return Srs<C>::template group_ntt_host<typename C::Fq2>(points, log_n, inverse, out);
}
template <class C>
int srs_generate_device(hipStream_t st, Arena& arena, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap,
                        const g16_srs_view* srs, const g16_params_view* out, double phase_ms[3]) {
    return Srs<C>::generate_device(st, arena, abc, ni, nc, nv, qap, srs, out, phase_ms);
}
template <class C>
int srs_generate_host(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap, const g16_srs_view* srs,
                      const g16_params_view* out) {
    return Srs<C>::generate_host(abc, ni, nc, nv, qap, srs, out);
}
template <class C>
int srs_queries_device(hipStream_t st, Arena& arena, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int log_n, const uint64_t* d_lag_g1,
                       const uint64_t* d_lag_g2, const g16_srs_view* fixed, const g16_params_view* out, double* products_ms) {
    return Srs<C>::queries_device(st, arena, abc, ni, nc, nv, log_n, d_lag_g1, d_lag_g2, fixed, out, products_ms);
}
template <class C>
int srs_queries_host(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, const uint64_t* u, const uint64_t* alpha_u, const uint64_t* beta_u,
                     const uint64_t* u_g2, const g16_srs_view* fixed, const g16_params_view* out) {
    typedef Affine<typename C::Fq> A1;
    G16_TRY(Srs<C>::check_matrices(abc, nc));
    G16_TRY(Srs<C>::queries_host(abc, ni, nc, nv, reinterpret_cast<const A1*>(u), reinterpret_cast<const A1*>(alpha_u), reinterpret_cast<const A1*>(beta_u),
                                 reinterpret_cast<const Affine<typename C::Fq2>*>(u_g2), out));
    Srs<C>::copy_fixed(fixed, out);
    return G16_OK;
}
template <class C>
int srs_apply_delta_device(hipStream_t st, Arena& arena, const uint64_t* delta, const g16_params_view* inout, uint64_t n_l, uint64_t n_h,
                           double* delta_ms) {
    return Srs<C>::apply_delta_device(st, arena, delta, inout, n_l, n_h, delta_ms);
}

#define G16_INSTANTIATE_SRS(C)                                                                                                             \
    template int srs_domain_log<C>(uint64_t, uint64_t, uint64_t, int, int*);                                                               \
    template int srs_group_ntt_device<C>(hipStream_t, Arena&, int, const uint64_t*, int, int, uint64_t*);                                  \
    template int srs_group_ntt_host<C>(int, const uint64_t*, int, int, uint64_t*);                                                         \
    template int srs_generate_device<C>(hipStream_t, Arena&, const g16_csr_view*, uint64_t, uint64_t, uint64_t, int, const g16_srs_view*,  \
                                        const g16_params_view*, double*);                                                                  \
    template int srs_generate_host<C>(const g16_csr_view*, uint64_t, uint64_t, uint64_t, int, const g16_srs_view*, const g16_params_view*); \
    template int srs_queries_device<C>(hipStream_t, Arena&, const g16_csr_view*, uint64_t, uint64_t, uint64_t, int, const uint64_t*,      \
                                       const uint64_t*, const g16_srs_view*, const g16_params_view*, double*);                             \
    template int srs_queries_host<C>(const g16_csr_view*, uint64_t, uint64_t, uint64_t, const uint64_t*, const uint64_t*, const uint64_t*,  \
                                     const uint64_t*, const g16_srs_view*, const g16_params_view*);                                        \
    template int srs_apply_delta_device<C>(hipStream_t, Arena&, const uint64_t*, const g16_params_view*, uint64_t, uint64_t, double*);
G16_INSTANTIATE_SRS(Bls12_381)
G16_INSTANTIATE_SRS(Bn254)

}  // namespace g16
