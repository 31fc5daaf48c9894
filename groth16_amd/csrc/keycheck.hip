// libg16_keycheck.so (include/g16_keycheck.h): is a proving key the key of (circuit, SRS) -- without deriving it again.
// A companion of the three other libraries, linked against them: this file holds the library's four kernels, the fold of the SRS
// under the circuit's matrices, the check, their host twins and the entry points.
//
// Every query of the derived key is a linear image of SRS points: a_query[j] = sum_i A~[i][j] L_i(tau) G with
// L_i(tau) G = n^-1 sum_k w^(-ik) T_k.  The transform matrix is symmetric, so for a coefficient vector rho over the variables
//     sum_j rho_j a_query[j] = sum_i (A~ rho)[i] L_i(tau) G = sum_k ifft_n(A~ rho)[k] T_k:
// a sparse mat-vec over ROWS (the prover's, with rho in the assignment's place), one scalar transform, one MSM with full-size scalars
// over the raw SRS points.  No transform over the group runs.  The pipeline:
//   upload matrices, rho, SRS prefixes, key -> membership of the key's points (verify_subgroup.hip's kernels; flags scanned on the host)
//   -> keycheck_rho_kernel -> keycheck_rows_kernel: six vectors (A, B, C) x (in, aux) -> ntt_dif_batch + bitrev_scale: six inverse
//   transforms -> keycheck_add_kernel: in + aux for A and B -> [Circom: keycheck_scatter_odd_kernel + one 2n-point transform]
//   -> sort_scalars per scalar vector (per-window plan: raw bases) -> convert_bases -> msm_bucket_pass + msm_reduce per sum
//   -> fold_windows on the host -> point compares and two-pair products (host templates).
//
//   keycheck_rho_kernel          one lane per coefficient: the two raw words -> Montgomery Fr (one product by R^2)
//   keycheck_rows_kernel         one lane per (row of the padded domain, matrix): spmv3_kernel's walk with TWO sums -- terms whose column
//                                is an instance variable go to `in`, the others to `aux`; A's rows nc .. nc + ni copy rho_in; rows
//                                above give zeros.  Gather-bound like spmv3_kernel
//   keycheck_scatter_odd_kernel  e[2j + 1] = rho_j, e[2j] = 0
//   keycheck_add_kernel          out = a + b
// The host twins run the same row walk (key_row_split), radix-2 transforms and a small bucket method in plain host C++.  The stage
// timers, the stream wait, uploads, Grp, flag -> reason, the bad-point record, pairs_equal, refuse, the checks of an SRS view and the
// stage times are ceremony_common.hpp's.
#include "ceremony_common.hpp"
#include "../../include/g16_keycheck.h"
#include "csr_row_dot.hpp"
#include "srs_setup.hpp"
#include <algorithm>

using namespace g16;

namespace g16 {

constexpr int KEYCHECK_BLOCK = 256;

// csr_row_dot (csr_row_dot.hpp) with the sum split by column: the same walk and the same coeff.is_one() fast path over the caller's
// (unmarked) arrays; a term of an instance variable (column < ni) is added to *in, every other to the local sum that *aux receives.
// *in is the caller's OUTPUT SLOT, zero on entry, and stays in memory through the walk: instance variables are few, so the slot is
// touched by a few terms of a few rows, and a lane holds spmv3_kernel's one accumulator, coefficient and operand -- not two sums
// (76 registers with both in registers against that kernel's 62; the parked form of spmv_circom_kernel, witness_map.hip)
template <class Fr>
G16_HD void key_row_split(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const Fr* __restrict__ val,
                          const Fr* __restrict__ rho, uint32_t ni, uint64_t row, Fr* in, Fr* aux) {
    Fr acc = Fr::zero();
    const Fr one = Fr::one();
    const uint64_t b = row_ptr[row];
    const uint32_t len = (uint32_t)(row_ptr[row + 1] - b);
    col += b;
    val += b;
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t c = col[k];
        const Fr coeff = val[k];
        const Fr v = rho[c];
        const Fr t = (coeff == one) ? v : v * coeff;
        if (c < ni) *in = *in + t;
        else acc = acc + t;
    }
    *aux = acc;
}

template <class Fr>
__global__ __launch_bounds__(KEYCHECK_BLOCK) void keycheck_rho_kernel(const uint64_t* __restrict__ coeffs, uint64_t n, Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * KEYCHECK_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = coeff_fr<Fr>(coeffs + 2 * i);
}

template <class Fr>
struct KeyRowArgs {
    const uint64_t* row_ptr[3];
    const uint32_t* col[3];
    const Fr* val[3];
    Fr* out_in[3];
    Fr* out_aux[3];
};
// blockIdx.y selects A / B / C (a domain has at most 2^30 rows: 32-bit row indices)
template <class Fr>
__global__ __launch_bounds__(KEYCHECK_BLOCK) void keycheck_rows_kernel(KeyRowArgs<Fr> args, const Fr* __restrict__ rho, uint32_t ni, uint32_t nc,
                                                                       uint32_t n) {
    const int m = blockIdx.y;
    const uint32_t row = blockIdx.x * KEYCHECK_BLOCK + threadIdx.x;
    if (row >= n) return;
    Fr* in = args.out_in[m] + row;
    Fr* aux = args.out_aux[m] + row;
    if (row < nc) {
        *in = Fr::zero();
        key_row_split<Fr>(args.row_ptr[m], args.col[m], args.val[m], rho, ni, row, in, aux);
    } else {
        *in = (m == 0 && row - nc < ni) ? rho[row - nc] : Fr::zero();   // the instance-copy rows of r1cs_to_qap.rs:195-199
        *aux = Fr::zero();
    }
}

template <class Fr>
__global__ __launch_bounds__(KEYCHECK_BLOCK) void keycheck_scatter_odd_kernel(const Fr* __restrict__ rho, uint64_t n, Fr* __restrict__ e) {
    const uint64_t j = (uint64_t)blockIdx.x * KEYCHECK_BLOCK + threadIdx.x;
    if (j >= n) return;
    e[2 * j] = Fr::zero();
    e[2 * j + 1] = rho[j];
}

template <class Fr>
__global__ __launch_bounds__(KEYCHECK_BLOCK) void keycheck_add_kernel(const Fr* __restrict__ a, const Fr* __restrict__ b, uint64_t n,
                                                                      Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * KEYCHECK_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = a[i] + b[i];
}

namespace {

inline unsigned kc_blocks(uint64_t n) { return (unsigned)((n + KEYCHECK_BLOCK - 1) / KEYCHECK_BLOCK); }

typedef StageTimes<g16_keycheck_timings, 10> Stages;

struct Shape {
    uint64_t ni, nc, nv, n, n_l, n_h, m;   // m: coefficients the call reads = max(nv, n_h)
    int log_n, qap;
    bool circom() const { return qap == G16_QAP_CIRCOM; }
};

// the six sums of one side of the equations
template <class C>
struct KeySums {
    typename C::G1A a, b1, gabc, l, h;
    typename C::G2A b2;
    KeySums() : a(C::G1A::identity()), b1(C::G1A::identity()), gabc(C::G1A::identity()), l(C::G1A::identity()), h(C::G1A::identity()),
                b2(C::G2A::identity()) {}
};

struct CallTimers {
    Timers upload, membership, rows, transforms, sorts, passes, reductions;
    double pairings = 0, c = 0, W = 0;
    void store(g16_keycheck_timings* tm) {
        tm->upload_ms = upload.total(); tm->membership_ms = membership.total(); tm->rows_ms = rows.total();
        tm->transforms_ms = transforms.total(); tm->sorts_ms = sorts.total(); tm->passes_ms = passes.total();
        tm->reductions_ms = reductions.total(); tm->pairings_ms = pairings; tm->window_bits = c; tm->windows = W;
    }
};

template <class F>
XYZZ<F> lift(const Affine<F>& p) { return XYZZ<F>::from_affine(p); }

// ---- host arithmetic ------------------------------------------------------------------------------------------------------------
template <class C>
typename C::Fr root_of(int log_n) {
    typename C::Fr w = C::two_adic_root();
    for (int k = log_n; k < C::TWO_ADICITY; ++k) w = w.sqr();
    return w;
}
// in place, natural order in and out, n^-1 included: bit reversal, then decimation-in-time butterflies over w^-1
template <class C>
void host_ifft(std::vector<typename C::Fr>& x, int log_n) {
    typedef typename C::Fr Fr;
    const uint64_t n = (uint64_t)1 << log_n;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t r = 0;
        for (int b = 0; b < log_n; ++b) r |= ((i >> b) & 1) << (log_n - 1 - b);
        if (r > i) std::swap(x[i], x[r]);
    }
    for (int s = 1; s <= log_n; ++s) {
        const uint64_t half = (uint64_t)1 << (s - 1);
        const Fr wm = root_of<C>(s).inverse();
        for (uint64_t lo = 0; lo < n; lo += 2 * half) {
            Fr w = Fr::one();
            for (uint64_t k = 0; k < half; ++k) {
                const Fr u = x[lo + k], t = x[lo + k + half] * w;
                x[lo + k] = u + t;
                x[lo + k + half] = u - t;
                w = w * wm;
            }
        }
    }
    const Fr n_inv = Fr::from_u64(n).inverse();
    for (auto& v : x) v = v * n_inv;
}
// sum_{i<n} sc[i] bases[i]: the bucket method over the canonical scalars, 4-bit windows for a few points and 8-bit windows for many
template <class F, class Fr>
Affine<F> host_msm(const Affine<F>* bases, const Fr* sc, uint64_t n) {
    const int cb = n <= 256 ? 4 : 8, per_word = 32 / cb;
    const uint32_t mask = (1u << cb) - 1u;
    std::vector<uint32_t> k(n * Fr::N);
    for (uint64_t i = 0; i < n; ++i) sc[i].to_canonical(k.data() + i * Fr::N);
    XYZZ<F> total = XYZZ<F>::identity();
    std::vector<XYZZ<F>> bucket(mask);
    for (int w = per_word * Fr::N - 1; w >= 0; --w) {
        for (int d = 0; d < cb; ++d) total = total.dbl();
        for (auto& b : bucket) b = XYZZ<F>::identity();
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t digit = (k[i * Fr::N + w / per_word] >> (cb * (w % per_word))) & mask;
            if (digit) bucket[digit - 1].add(lift(bases[i]));
        }
        XYZZ<F> run = XYZZ<F>::identity(), sum = XYZZ<F>::identity();
        for (int b = (int)mask - 1; b >= 0; --b) {
            run.add(bucket[b]);
            sum.add(run);
        }
        total.add(sum);
    }
    return total.to_affine();
}
// the same over `count` points in caller memory (8-byte aligned words): sum_{i<count} sc[i] pts[i]
template <class F, class Fr>
Affine<F> host_msm_words(const uint64_t* pts, uint64_t count, const Fr* sc) {
    std::vector<Affine<F>> copy(count);
    if (count) memcpy(copy.data(), pts, count * sizeof(Affine<F>));
    return host_msm<F, Fr>(copy.data(), sc, count);
}
template <class F>
Affine<F> add3(const Affine<F>& a, const Affine<F>& b, const Affine<F>& c) {
    XYZZ<F> s = lift(a);
    s.add(lift(b));
    s.add(lift(c));
    return s.to_affine();
}
template <class F>
Affine<F> sub2(const Affine<F>& a, const Affine<F>& b) {
    XYZZ<F> s = lift(a);
    s.add(lift(b.neg()));
    return s.to_affine();
}

// the first bad point of one array of a key in host memory (flags as the membership kernels write them: 1 in, 2 off the curve, 0 out)
void scan_flags(const std::vector<uint8_t>& flags, uint32_t array, unsigned long long* rec) {
    if (*rec != BAD_NONE) return;
    for (uint64_t i = 0; i < flags.size(); ++i)
        if (const uint32_t reason = flag_reason(flags[i], true)) {   // the identity is a point of a query
            *rec = bad_key(array, i, reason);
            return;
        }
}
template <class C, int G2>
void host_flags(const uint64_t* pts, uint64_t n, std::vector<uint8_t>& flags) {
    typedef Grp<C, G2> G;
    flags.resize(n);
    for (uint64_t i = 0; i < n; ++i) flags[i] = G::flag(ld_any<typename G::A>(pts + i * G::WORDS));
}
// the two deltas: on the host in both forms (two points); the identity is refused
template <class C>
void check_deltas(const g16_params_view* key, unsigned long long* rec) {
    if (*rec != BAD_NONE) return;
    const uint32_t r1 = point_reason<C, 0>(ld_any<typename C::G1A>(key->delta_g1), false);
    const uint32_t r2 = point_reason<C, 1>(ld_any<typename C::G2A>(key->delta_g2), false);
    if (r1) *rec = bad_key(6, 0, r1);
    else if (r2) *rec = bad_key(7, 0, r2);
}

// ---- the host twin ----------------------------------------------------------------------------------------------------------------
template <class C>
int fold_host(const Shape& sh, const g16_csr_view abc[3], const g16_srs_view* srs, const g16_params_view* key, const uint64_t* rho128,
              KeySums<C>* s_srs, KeySums<C>* s_key, unsigned long long* bad) {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef typename C::G1A A1;
    typedef typename C::G2A A2;
    const uint64_t n = sh.n;
    *bad = BAD_NONE;
    if (key) {
        std::vector<uint8_t> fl;
        const struct { const void* p; uint64_t cnt; int g2; } arr[6] = {{key->a_query, sh.nv, 0},      {key->b_g1_query, sh.nv, 0},
                                                                        {key->b_g2_query, sh.nv, 1},   {key->gamma_abc_g1, sh.ni, 0},
                                                                        {key->l_query, sh.n_l, 0},     {key->h_query, sh.n_h, 0}};
        for (uint32_t k = 0; k < 6; ++k) {
            if (arr[k].g2) host_flags<C, 1>((const uint64_t*)arr[k].p, arr[k].cnt, fl);
            else host_flags<C, 0>((const uint64_t*)arr[k].p, arr[k].cnt, fl);
            scan_flags(fl, k, bad);
        }
        check_deltas<C>(key, bad);
        if (*bad != BAD_NONE) return G16_OK;
    }
    std::vector<Fr> rho(sh.m);
    for (uint64_t i = 0; i < sh.m; ++i) rho[i] = coeff_fr<Fr>(rho128 + 2 * i);
    // w[2 m] = w_M(rho_in), w[2 m + 1] = w_M(rho_aux)
    std::vector<Fr> w[6];
    for (int m = 0; m < 3; ++m) {
        std::vector<Fr>&in = w[2 * m], &aux = w[2 * m + 1];
        in.assign(n, Fr::zero());
        aux.assign(n, Fr::zero());
        for (uint64_t row = 0; row < sh.nc; ++row)
            key_row_split<Fr>(abc[m].row_ptr, abc[m].col, reinterpret_cast<const Fr*>(abc[m].val), rho.data(), (uint32_t)sh.ni, row, &in[row],
                              &aux[row]);
        if (m == 0) for (uint64_t j = 0; j < sh.ni; ++j) in[sh.nc + j] = rho[j];
        host_ifft<C>(in, sh.log_n);
        host_ifft<C>(aux, sh.log_n);
    }
    std::vector<Fr> wa(n), wb(n);
    for (uint64_t i = 0; i < n; ++i) { wa[i] = w[0][i] + w[1][i]; wb[i] = w[2][i] + w[3][i]; }
    // the SRS prefixes as aligned copies
    std::vector<A1> t1(2 * n - 1), al(n), be(n);
    std::vector<A2> t2(n);
    memcpy(t1.data(), srs->tau_g1, t1.size() * sizeof(A1));
    memcpy(al.data(), srs->alpha_tau_g1, n * sizeof(A1));
    memcpy(be.data(), srs->beta_tau_g1, n * sizeof(A1));
    memcpy(t2.data(), srs->tau_g2, n * sizeof(A2));
    s_srs->a = host_msm<Fq, Fr>(t1.data(), wa.data(), n);
    s_srs->b1 = host_msm<Fq, Fr>(t1.data(), wb.data(), n);
    s_srs->b2 = host_msm<Fq2, Fr>(t2.data(), wb.data(), n);
    s_srs->gabc = add3(host_msm<Fq, Fr>(be.data(), w[0].data(), n), host_msm<Fq, Fr>(al.data(), w[2].data(), n),
                       host_msm<Fq, Fr>(t1.data(), w[4].data(), n));
    if (sh.n_l)
        s_srs->l = add3(host_msm<Fq, Fr>(be.data(), w[1].data(), n), host_msm<Fq, Fr>(al.data(), w[3].data(), n),
                        host_msm<Fq, Fr>(t1.data(), w[5].data(), n));
    if (sh.circom()) {
        std::vector<Fr> e(2 * n, Fr::zero());
        for (uint64_t j = 0; j < n; ++j) e[2 * j + 1] = rho[j];
        host_ifft<C>(e, sh.log_n + 1);
        s_srs->h = host_msm<Fq, Fr>(t1.data(), e.data(), 2 * n - 1);
    } else if (sh.n_h) {
        s_srs->h = sub2(host_msm<Fq, Fr>(t1.data() + n, rho.data(), sh.n_h), host_msm<Fq, Fr>(t1.data(), rho.data(), sh.n_h));
    }
    if (key) {
        s_key->a = host_msm_words<Fq, Fr>((const uint64_t*)key->a_query, sh.nv, rho.data());
        s_key->b1 = host_msm_words<Fq, Fr>((const uint64_t*)key->b_g1_query, sh.nv, rho.data());
        s_key->b2 = host_msm_words<Fq2, Fr>((const uint64_t*)key->b_g2_query, sh.nv, rho.data());
        s_key->gabc = host_msm_words<Fq, Fr>(key->gamma_abc_g1, sh.ni, rho.data());
        if (sh.n_l) s_key->l = host_msm_words<Fq, Fr>((const uint64_t*)key->l_query, sh.n_l, rho.data() + sh.ni);
        if (sh.n_h) s_key->h = host_msm_words<Fq, Fr>((const uint64_t*)key->h_query, sh.n_h, rho.data());
    }
    return G16_OK;
}

// ---- the device form --------------------------------------------------------------------------------------------------------------
// one sum waiting for the stream: the window sums land in hws (its storage does not move: a deque element), fold() after the wait
template <class F>
struct Pending {
    std::vector<XYZZ<F>> hws;
    MsmPlan plan;
    Affine<F> value = Affine<F>::identity();
    void fold() { if (!hws.empty()) value = fold_windows<F>(hws.data(), plan).to_affine(); }
};
// sum over the sort's entries p with 0 <= p + shift < base_count of scalar_p bases[p + shift]; base_count = 0: the identity, no launch
template <class F>
int enqueue_sum(const CeremonyEnv& env, const Affine<F>* d_bases, int64_t shift, uint64_t base_count, const ScalarSort& ss, std::deque<Pending<F>>& q,
                Pending<F>** out, CallTimers& ct) {
    q.emplace_back();
    Pending<F>& p = q.back();
    *out = &p;
    if (!base_count) return G16_OK;
    p.plan = ss.plan;
    p.hws.resize(ss.plan.outputs());
    MsmBuffers<F> buf;
    G16_TRY((msm_bucket_pass<F>(d_bases, shift, base_count, ss, *env.arena, env.st, &buf, ct.passes.add())));
    EventTimer* tr = ct.reductions.add();
    G16_TRY(tr->start(env.st));
    G16_TRY((msm_reduce<F>(buf, ss, env.st)));
    G16_TRY(tr->stop(env.st));
    G16_HIP_TRY(hipMemcpyAsync(p.hws.data(), buf.window_sums, sizeof(XYZZ<F>) * p.hws.size(), hipMemcpyDeviceToHost, env.st));
    return G16_OK;
}

template <class C>
struct DomainHold {
    Domain<C>* d = nullptr;
    ~DomainHold() { domain_destroy<C>(d); }
};

template <class C, int G2>
int device_flags(const CeremonyEnv& env, const typename Grp<C, G2>::A* d_pts, uint64_t n, std::vector<uint8_t>& host) {
    host.assign(n, 1);
    if (!n) return G16_OK;
    uint8_t* d_flags = nullptr;
    G16_TRY(env.arena->alloc_n(n, &d_flags));
    G16_TRY(subgroup_enqueue_points(env.st, C::CURVE_ID, G2, reinterpret_cast<const uint64_t*>(d_pts), n, d_flags));
    G16_HIP_TRY(hipMemcpyAsync(host.data(), d_flags, n, hipMemcpyDeviceToHost, env.st));
    return G16_OK;
}

template <class C>
int fold_device(const CeremonyEnv& env, const Shape& sh, const g16_csr_view abc[3], const g16_srs_view* srs, const g16_params_view* key,
                const uint64_t* rho128, KeySums<C>* s_srs, KeySums<C>* s_key, unsigned long long* bad, CallTimers& ct) {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef typename C::G1A A1;
    typedef typename C::G2A A2;
    const uint64_t n = sh.n, n_tau = 2 * n - 1;
    const hipStream_t st = env.st;
    *bad = BAD_NONE;
    DomainHold<C> dom, dom2;   // destroyed after the stream has drained (StreamWait is declared later, so it runs first)
    StreamWait wait{st};
    // ---- upload
    KeyRowArgs<Fr> ra;
    uint64_t* d_rho128 = nullptr;
    A1 *d_t1 = nullptr, *d_al = nullptr, *d_be = nullptr, *k_a = nullptr, *k_b1 = nullptr, *k_g = nullptr, *k_l = nullptr, *k_h = nullptr;
    A2 *d_t2 = nullptr, *k_b2 = nullptr;
    EventTimer* tu = ct.upload.add();
    G16_TRY(tu->start(st));
    for (int m = 0; m < 3; ++m) {
        const uint64_t end = abc[m].row_ptr[sh.nc];
        uint64_t* rp = nullptr;
        uint32_t* cl = nullptr;
        Fr* vl = nullptr;
        G16_TRY(upload<uint64_t>(env, abc[m].row_ptr, sh.nc + 1, &rp));
        G16_TRY(upload<uint32_t>(env, abc[m].col, end, &cl));
        G16_TRY(upload<Fr>(env, abc[m].val, end, &vl));
        ra.row_ptr[m] = rp; ra.col[m] = cl; ra.val[m] = vl;
    }
    G16_TRY(upload<uint64_t>(env, rho128, 2 * sh.m, &d_rho128));
    G16_TRY(upload<A1>(env, srs->tau_g1, n_tau, &d_t1));
    G16_TRY(upload<A2>(env, srs->tau_g2, n, &d_t2));
    G16_TRY(upload<A1>(env, srs->alpha_tau_g1, n, &d_al));
    G16_TRY(upload<A1>(env, srs->beta_tau_g1, n, &d_be));
    if (key) {
        G16_TRY(upload<A1>(env, key->a_query, sh.nv, &k_a));
        G16_TRY(upload<A1>(env, key->b_g1_query, sh.nv, &k_b1));
        G16_TRY(upload<A2>(env, key->b_g2_query, sh.nv, &k_b2));
        G16_TRY(upload<A1>(env, key->gamma_abc_g1, sh.ni, &k_g));
        G16_TRY(upload<A1>(env, key->l_query, sh.n_l, &k_l));
        G16_TRY(upload<A1>(env, key->h_query, sh.n_h, &k_h));
    }
    G16_TRY(tu->stop(st));
    // ---- membership of the key's points, on the uploaded copies
    if (key) {
        std::vector<uint8_t> fl[6];
        EventTimer* tm = ct.membership.add();
        G16_TRY(tm->start(st));
        G16_TRY((device_flags<C, 0>(env, k_a, sh.nv, fl[0])));
        G16_TRY((device_flags<C, 0>(env, k_b1, sh.nv, fl[1])));
        G16_TRY((device_flags<C, 1>(env, k_b2, sh.nv, fl[2])));
        G16_TRY((device_flags<C, 0>(env, k_g, sh.ni, fl[3])));
        G16_TRY((device_flags<C, 0>(env, k_l, sh.n_l, fl[4])));
        G16_TRY((device_flags<C, 0>(env, k_h, sh.n_h, fl[5])));
        G16_TRY(tm->stop(st));
        G16_HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < 6; ++k) scan_flags(fl[k], k, bad);
        check_deltas<C>(key, bad);
        if (*bad != BAD_NONE) return G16_OK;
    }
    // ---- rows: rho as Fr, then the six row vectors
    Fr* d_rho = nullptr;
    Fr* v[6];    // (A, B, C) x (in, aux): the row sums, bit-reversed after the transform
    Fr* w[6];    // their inverse transforms, natural order
    Fr *wa = nullptr, *wb = nullptr, *e_in = nullptr, *e_out = nullptr;
    G16_TRY(env.arena->alloc_n(sh.m, &d_rho));
    for (int k = 0; k < 6; ++k) {
        G16_TRY(env.arena->alloc_n(n, &v[k]));
        G16_TRY(env.arena->alloc_n(n, &w[k]));
    }
    G16_TRY(env.arena->alloc_n(n, &wa));
    G16_TRY(env.arena->alloc_n(n, &wb));
    for (int m = 0; m < 3; ++m) { ra.out_in[m] = v[2 * m]; ra.out_aux[m] = v[2 * m + 1]; }
    EventTimer* trw = ct.rows.add();
    G16_TRY(trw->start(st));
    hipLaunchKernelGGL((keycheck_rho_kernel<Fr>), dim3(kc_blocks(sh.m)), dim3(KEYCHECK_BLOCK), 0, st, d_rho128, sh.m, d_rho);
    G16_LAUNCH_CHECK();
    hipLaunchKernelGGL((keycheck_rows_kernel<Fr>), dim3(kc_blocks(n), 3), dim3(KEYCHECK_BLOCK), 0, st, ra, d_rho, (uint32_t)sh.ni, (uint32_t)sh.nc,
                       (uint32_t)n);
    G16_LAUNCH_CHECK();
    G16_TRY(trw->stop(st));
    // ---- transforms: six n-point inverses (three chains per launch), in + aux for A and B, the Circom h vector
    EventTimer* tt = ct.transforms.add();
    G16_TRY(tt->start(st));
    G16_TRY((domain_create<C>(sh.log_n, st, &dom.d, false)));
    G16_TRY((ntt_dif_batch<C>(dom.d, &v[0], 3, true, st)));
    G16_TRY((ntt_dif_batch<C>(dom.d, &v[3], 3, true, st)));
    for (int k = 0; k < 6; ++k) G16_TRY((bitrev_scale<C>(dom.d, w[k], v[k], nullptr, &dom.d->n_inv, st)));
    hipLaunchKernelGGL((keycheck_add_kernel<Fr>), dim3(kc_blocks(n)), dim3(KEYCHECK_BLOCK), 0, st, w[0], w[1], n, wa);
    G16_LAUNCH_CHECK();
    hipLaunchKernelGGL((keycheck_add_kernel<Fr>), dim3(kc_blocks(n)), dim3(KEYCHECK_BLOCK), 0, st, w[2], w[3], n, wb);
    G16_LAUNCH_CHECK();
    if (sh.circom()) {
        G16_TRY(env.arena->alloc_n(2 * n, &e_in));
        G16_TRY(env.arena->alloc_n(2 * n, &e_out));
        G16_TRY((domain_create<C>(sh.log_n + 1, st, &dom2.d, false)));
        hipLaunchKernelGGL((keycheck_scatter_odd_kernel<Fr>), dim3(kc_blocks(n)), dim3(KEYCHECK_BLOCK), 0, st, d_rho, n, e_in);
        G16_LAUNCH_CHECK();
        G16_TRY((ntt_dif<C>(dom2.d, e_in, true, st)));
        G16_TRY((bitrev_scale<C>(dom2.d, e_out, e_in, nullptr, &dom2.d->n_inv, st)));
    }
    G16_TRY(tt->stop(st));
    // ---- sorts: one per scalar vector
    ScalarSort s_a, s_b, s_w[6], s_rho, s_e;
    auto sort = [&](const Fr* d, uint64_t cnt, ScalarSort* ss) -> int {
        EventTimer* ts = ct.sorts.add();
        G16_TRY(ts->start(st));
        G16_TRY((sort_scalars<C>(d, cnt, 0, *env.arena, st, ss)));
        return ts->stop(st);
    };
    G16_TRY(sort(wa, n, &s_a));
    G16_TRY(sort(wb, n, &s_b));
    for (int k = 0; k < 6; ++k)
        if (k % 2 == 0 || sh.n_l) G16_TRY(sort(w[k], n, &s_w[k]));
    if (key || (!sh.circom() && sh.n_h)) G16_TRY(sort(d_rho, sh.m, &s_rho));
    if (sh.circom()) G16_TRY(sort(e_out, n_tau, &s_e));
    ct.c = s_a.plan.c;
    ct.W = s_a.plan.W;
    // ---- the bases in the bucket kernel's radix, in place
    G16_TRY((convert_bases<Fq>(d_t1, n_tau, st)));
    G16_TRY((convert_bases<Fq2>(d_t2, n, st)));
    G16_TRY((convert_bases<Fq>(d_al, n, st)));
    G16_TRY((convert_bases<Fq>(d_be, n, st)));
    if (key) {
        G16_TRY((convert_bases<Fq>(k_a, sh.nv, st)));
        G16_TRY((convert_bases<Fq>(k_b1, sh.nv, st)));
        G16_TRY((convert_bases<Fq2>(k_b2, sh.nv, st)));
        G16_TRY((convert_bases<Fq>(k_g, sh.ni, st)));
        if (sh.n_l) G16_TRY((convert_bases<Fq>(k_l, sh.n_l, st)));
        if (sh.n_h) G16_TRY((convert_bases<Fq>(k_h, sh.n_h, st)));
    }
    // ---- the sums
    std::deque<Pending<Fq>> q1;
    std::deque<Pending<Fq2>> q2;
    Pending<Fq>*p_a, *p_b1, *p_g[3], *p_l[3] = {nullptr, nullptr, nullptr}, *p_h[2] = {nullptr, nullptr};
    Pending<Fq>*pk_a = nullptr, *pk_b1 = nullptr, *pk_g = nullptr, *pk_l = nullptr, *pk_h = nullptr;
    Pending<Fq2>*p_b2, *pk_b2 = nullptr;
    G16_TRY((enqueue_sum<Fq>(env, d_t1, 0, n, s_a, q1, &p_a, ct)));
    G16_TRY((enqueue_sum<Fq>(env, d_t1, 0, n, s_b, q1, &p_b1, ct)));
    G16_TRY((enqueue_sum<Fq2>(env, d_t2, 0, n, s_b, q2, &p_b2, ct)));
    G16_TRY((enqueue_sum<Fq>(env, d_be, 0, n, s_w[0], q1, &p_g[0], ct)));
    G16_TRY((enqueue_sum<Fq>(env, d_al, 0, n, s_w[2], q1, &p_g[1], ct)));
    G16_TRY((enqueue_sum<Fq>(env, d_t1, 0, n, s_w[4], q1, &p_g[2], ct)));
    if (sh.n_l) {
        G16_TRY((enqueue_sum<Fq>(env, d_be, 0, n, s_w[1], q1, &p_l[0], ct)));
        G16_TRY((enqueue_sum<Fq>(env, d_al, 0, n, s_w[3], q1, &p_l[1], ct)));
        G16_TRY((enqueue_sum<Fq>(env, d_t1, 0, n, s_w[5], q1, &p_l[2], ct)));
    }
    if (sh.circom()) {
        G16_TRY((enqueue_sum<Fq>(env, d_t1, 0, n_tau, s_e, q1, &p_h[0], ct)));
    } else if (sh.n_h) {
        // entry p < n - 1 reads tau_g1[p + n] (the array ends at 2n - 1) and tau_g1[p]
        G16_TRY((enqueue_sum<Fq>(env, d_t1, (int64_t)n, n_tau, s_rho, q1, &p_h[0], ct)));
        G16_TRY((enqueue_sum<Fq>(env, d_t1, 0, sh.n_h, s_rho, q1, &p_h[1], ct)));
    }
    if (key) {
        G16_TRY((enqueue_sum<Fq>(env, k_a, 0, sh.nv, s_rho, q1, &pk_a, ct)));
        G16_TRY((enqueue_sum<Fq>(env, k_b1, 0, sh.nv, s_rho, q1, &pk_b1, ct)));
        G16_TRY((enqueue_sum<Fq2>(env, k_b2, 0, sh.nv, s_rho, q2, &pk_b2, ct)));
        G16_TRY((enqueue_sum<Fq>(env, k_g, 0, sh.ni, s_rho, q1, &pk_g, ct)));
        G16_TRY((enqueue_sum<Fq>(env, k_l, -(int64_t)sh.ni, sh.n_l, s_rho, q1, &pk_l, ct)));   // entry j >= ni reads l_query[j - ni]
        G16_TRY((enqueue_sum<Fq>(env, k_h, 0, sh.n_h, s_rho, q1, &pk_h, ct)));
    }
    G16_HIP_TRY(hipStreamSynchronize(st));
    for (auto& p : q1) p.fold();
    for (auto& p : q2) p.fold();
    s_srs->a = p_a->value;
    s_srs->b1 = p_b1->value;
    s_srs->b2 = p_b2->value;
    s_srs->gabc = add3(p_g[0]->value, p_g[1]->value, p_g[2]->value);
    if (sh.n_l) s_srs->l = add3(p_l[0]->value, p_l[1]->value, p_l[2]->value);
    if (sh.circom()) s_srs->h = p_h[0]->value;
    else if (sh.n_h) s_srs->h = sub2(p_h[0]->value, p_h[1]->value);
    if (key) {
        s_key->a = pk_a->value; s_key->b1 = pk_b1->value; s_key->b2 = pk_b2->value;
        s_key->gabc = pk_g->value; s_key->l = pk_l->value; s_key->h = pk_h->value;
    }
    return G16_OK;
}

// ---- arguments ------------------------------------------------------------------------------------------------------------------------
// the shape of the call, the matrices (every column below num_variables: the row kernel gathers by them), the SRS lengths the
// equations need, the coefficients
template <class C>
int check_args(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap, const g16_srs_view* srs, const uint64_t* coeffs,
               uint64_t n_coeffs, Shape* sh) {
    int log_n = 0;
    G16_TRY(srs_domain_log<C>(ni, nc, nv, qap, &log_n));
    const uint64_t n = (uint64_t)1 << log_n;
    if (nv >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
    *sh = Shape{ni, nc, nv, n, nv - ni, qap == G16_QAP_CIRCOM ? n : n - 1, 0, log_n, qap};
    sh->m = std::max(nv, sh->n_h);
    for (int m = 0; m < 3; ++m) {
        const g16_csr_view& v = abc[m];
        if (!v.row_ptr) return G16_ERR_BAD_ARG;
        for (uint64_t i = 0; i < nc; ++i)
            if (v.row_ptr[i] > v.row_ptr[i + 1]) return G16_ERR_BAD_LENGTH;
        if ((!v.col || !v.val) && v.row_ptr[nc]) return G16_ERR_BAD_ARG;
        if (v.row_ptr[nc] >= ((uint64_t)1 << 32)) return G16_ERR_BAD_LENGTH;
        for (uint64_t k = v.row_ptr[0]; k < v.row_ptr[nc]; ++k)
            if (v.col[k] >= nv) return refuse(G16_ERR_BAD_LENGTH, "key check%s: matrix %llu names column %llu of %llu variables", m, v.col[k], nv);
    }
    if (!srs_view_ok(srs)) return G16_ERR_BAD_ARG;
    const SrsArray arr[3] = {
        {"tau_g1", srs->n_tau_g1, 2 * n - 1}, {"tau_g2", srs->n_tau_g2, n}, {"alpha_tau_g1 / beta_tau_g1 (one count)", srs->n_alpha_beta, n}};
    // srs_lengths passes (name, have, need, n): the text names them in another order, hence the positions
    G16_TRY(srs_lengths(arr, "SRS too short: %1$s holds %2$llu points, a domain of %4$llu needs %3$llu", n));
    if (coeffs && n_coeffs < sh->m)
        return refuse(G16_ERR_BAD_LENGTH, "key check%s: %llu coefficients, %llu variables and %llu points of h_query need more", n_coeffs, nv, sh->n_h);
    return G16_OK;
}

bool key_view_ok(const g16_params_view* k, const Shape& sh) {
    if (!k->alpha_g1 || !k->beta_g1 || !k->delta_g1 || !k->beta_g2 || !k->delta_g2 || !k->gamma_g2) return false;
    if (k->flags & G16_PARAMS_DEVICE_PTRS) return false;
    return k->gamma_abc_g1 && k->a_query && k->b_g1_query && k->b_g2_query && (k->h_query || !sh.n_h) && (k->l_query || !sh.n_l);
}

}  // namespace

// key == nullptr: the fold alone (out receives the SRS side); else the check (info receives the verdict)
template <class C>
int keycheck_any(const CeremonyEnv* env, g16_keycheck_timings* tm, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap,
                 const g16_srs_view* srs, const g16_params_view* key, const uint64_t* coeffs, uint64_t n_coeffs, const g16_key_fold* out,
                 g16_ceremony_info* info) {
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    if (info) *info = g16_ceremony_info{};
    if (tm) *tm = g16_keycheck_timings{};
    Shape sh;
    G16_TRY(check_args<C>(abc, ni, nc, nv, qap, srs, coeffs, n_coeffs, &sh));
    if (key && !key_view_ok(key, sh)) return G16_ERR_BAD_ARG;
    std::vector<uint64_t> own;
    const uint64_t* rho = nullptr;
    G16_TRY(agg_coeffs(coeffs, sh.m, own, &rho));
    KeySums<C> s_srs, s_key;
    unsigned long long bad = BAD_NONE;
    if (env) {
        CallTimers ct;
        const int rc = fold_device<C>(*env, sh, abc, srs, key, rho, &s_srs, &s_key, &bad, ct);
        ct.store(tm);
        G16_TRY(rc);
    } else {
        G16_TRY(fold_host<C>(sh, abc, srs, key, rho, &s_srs, &s_key, &bad));
    }
    if (!key) {
        memcpy(out->a, &s_srs.a, sizeof(G1A));
        memcpy(out->b_g1, &s_srs.b1, sizeof(G1A));
        memcpy(out->b_g2, &s_srs.b2, sizeof(G2A));
        memcpy(out->gamma_abc, &s_srs.gabc, sizeof(G1A));
        memcpy(out->l, &s_srs.l, sizeof(G1A));
        memcpy(out->h, &s_srs.h, sizeof(G1A));
        return G16_OK;
    }
    if (bad != BAD_NONE) { decode_bad(bad, G16_KEYCHECK_BAD_POINT, info); return G16_OK; }
    uint32_t flags = 0;
    const struct { const uint64_t *a, *b; size_t bytes; } fixed[4] = {{key->alpha_g1, srs->alpha_tau_g1, sizeof(G1A)},
                                                                      {key->beta_g1, srs->beta_tau_g1, sizeof(G1A)},
                                                                      {key->beta_g2, srs->beta_g2, sizeof(G2A)},
                                                                      {key->gamma_g2, srs->tau_g2, sizeof(G2A)}};
    for (uint32_t k = 0; k < 4; ++k)
        if (memcmp(fixed[k].a, fixed[k].b, fixed[k].bytes) != 0) {
            flags |= G16_KEYCHECK_FIXED;
            info->bad_array = k;
            break;
        }
    if (!(s_key.a == s_srs.a)) flags |= G16_KEYCHECK_A;
    if (!(s_key.b1 == s_srs.b1)) flags |= G16_KEYCHECK_B_G1;
    if (!(s_key.b2 == s_srs.b2)) flags |= G16_KEYCHECK_B_G2;
    if (!(s_key.gabc == s_srs.gabc)) flags |= G16_KEYCHECK_GAMMA_ABC;
    const G1A g1 = ld_any<G1A>(srs->tau_g1), d1 = ld_any<G1A>(key->delta_g1);
    const G2A g2 = ld_any<G2A>(srs->tau_g2), d2 = ld_any<G2A>(key->delta_g2);
    const double t0 = wall_ms();
    bool eq = true;
    G16_TRY(pairs_equal<C>(d1, g2, g1, d2, &eq));
    if (!eq) flags |= G16_KEYCHECK_DELTA;
    if (sh.n_l) {
        G16_TRY(pairs_equal<C>(s_key.l, d2, s_srs.l, g2, &eq));
        if (!eq) flags |= G16_KEYCHECK_L;
    }
    if (sh.n_h) {
        G16_TRY(pairs_equal<C>(s_key.h, d2, s_srs.h, g2, &eq));
        if (!eq) flags |= G16_KEYCHECK_H;
    }
    if (tm) tm->pairings_ms = wall_ms() - t0;
    info->flags = flags;
    return G16_OK;
}

}  // namespace g16

extern "C" {

int g16_params_check_derivation(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables,
                                int qap, const g16_srs_view* srs, const g16_params_view* key, const uint64_t* coeffs, uint64_t n_coeffs,
                                g16_ceremony_info* info) {
    if (!ctx || !abc || !srs || !key || !info) return G16_ERR_BAD_ARG;
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    g16_keycheck_timings* tm = Stages::of(keycheck_stage_ms(ctx));
    G16_VERIFY_DISPATCH(curve, (keycheck_any<CC>(&env, tm, abc, num_inputs, num_constraints, num_variables, qap, srs, key, coeffs, n_coeffs, nullptr,
                                                 info)));
}

int g16_host_params_check_derivation(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                     uint64_t num_variables, int qap, const g16_srs_view* srs, const g16_params_view* key,
                                     const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info) {
    if (!abc || !srs || !key || !info) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(curve, (keycheck_any<CC>(nullptr, nullptr, abc, num_inputs, num_constraints, num_variables, qap, srs, key, coeffs, n_coeffs,
                                                 nullptr, info)));
}

static bool fold_out_ok(const g16_key_fold* o) { return o && o->a && o->b_g1 && o->b_g2 && o->gamma_abc && o->l && o->h; }

int g16_key_fold_from_srs(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables, int qap,
                          const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, const g16_key_fold* out) {
    if (!ctx || !abc || !srs || !coeffs || !fold_out_ok(out)) return G16_ERR_BAD_ARG;
    CeremonyEnv env;
    int curve = -1;
    G16_TRY(ceremony_enter(ctx, &env, &curve));
    g16_keycheck_timings* tm = Stages::of(keycheck_stage_ms(ctx));
    G16_VERIFY_DISPATCH(curve, (keycheck_any<CC>(&env, tm, abc, num_inputs, num_constraints, num_variables, qap, srs, nullptr, coeffs, n_coeffs, out,
                                                 nullptr)));
}

int g16_host_key_fold_from_srs(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables,
                               int qap, const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, const g16_key_fold* out) {
    if (!abc || !srs || !coeffs || !fold_out_ok(out)) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(curve, (keycheck_any<CC>(nullptr, nullptr, abc, num_inputs, num_constraints, num_variables, qap, srs, nullptr, coeffs,
                                                 n_coeffs, out, nullptr)));
}

int g16_keycheck_get_timings(g16_ctx* ctx, g16_keycheck_timings* out) {
    return Stages::get(keycheck_stage_ms(ctx), out);
}

}  // extern "C"
