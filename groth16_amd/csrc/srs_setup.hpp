// Trapdoor-free setup (srs_setup.hip): a circuit's proving key from a powers-of-tau SRS, and a delta contribution on top of it.
// The entry points of include/g16_mi355x.h ("setup from an SRS") are thin wrappers in api.hip over the functions declared here.
#pragma once
#include "internal.hpp"

namespace g16 {

// entries one lane of the sparse product walks at most (G16_SRS_SEGMENT_LEN; see srs_colsum_kernel)
static constexpr uint32_t SRS_SEGMENT_LEN = G16_SRS_SEGMENT_LEN;

// n = the power of two >= num_constraints + num_inputs, checked the way Setup::qap_evaluations checks it (plus D::new(2n) for Circom)
template <class C> int srs_domain_log(uint64_t ni, uint64_t nc, uint64_t nv, int qap, int* log_n);

// affine in, affine out, natural order on both sides; `inverse` includes n^-1.  points / out: host memory
template <class C> int srs_group_ntt_device(hipStream_t st, Arena& arena, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out);
template <class C> int srs_group_ntt_host(int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out);

// steps 1-3 of the derivation (gamma = delta = 1).  The SRS lengths have been checked by the caller; `out` holds host pointers.
// phase_ms (device form only, may be null): transforms, sparse products, h step -- stream events
template <class C> int srs_generate_device(hipStream_t st, Arena& arena, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap,
                                           const g16_srs_view* srs, const g16_params_view* out, double phase_ms[3]);
template <class C> int srs_generate_host(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int qap, const g16_srs_view* srs,
                                         const g16_params_view* out);

// The tail of the derivation alone (libg16_lagrange.so): the transposition, the segment plans, the sparse products and the copies out,
// from Lagrange points that are complete.  The matrices are checked here; log_n is the caller's to hold against the circuit.
// Device form: d_lag_g1 = u | alpha u | beta u (3n points, ONE array: the products index it as one), d_lag_g2 = u in G2 (n points),
// both in `arena`, which is not reset; it returns after the stream has drained.  Host form: four host arrays of n points.
// fixed: index 0 of tau_g1, alpha_tau_g1, beta_tau_g1, tau_g2 and beta_g2 is read (the key's single points); h_query is the caller's
template <class C> int srs_queries_device(hipStream_t st, Arena& arena, const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, int log_n,
                                          const uint64_t* d_lag_g1, const uint64_t* d_lag_g2, const g16_srs_view* fixed, const g16_params_view* out,
                                          double* products_ms);
template <class C> int srs_queries_host(const g16_csr_view abc[3], uint64_t ni, uint64_t nc, uint64_t nv, const uint64_t* u, const uint64_t* alpha_u,
                                        const uint64_t* beta_u, const uint64_t* u_g2, const g16_srs_view* fixed, const g16_params_view* out);

// step 4 in place: delta_g1, delta_g2 <- delta (.) on the host; the n_l + n_h points of l_query / h_query <- delta^-1 (.) on the GPU
template <class C> int srs_apply_delta_device(hipStream_t st, Arena& arena, const uint64_t* delta, const g16_params_view* inout, uint64_t n_l,
                                              uint64_t n_h, double* delta_ms);

// setup.hip (it owns the fixed-base kernels): tau^i g1 (n_tau_g1), tau^i g2, alpha tau^i g1, beta tau^i g1 (n_other each), beta g2
template <class C> int srs_from_trapdoor_device(hipStream_t st, Arena& arena, const uint64_t* tau, const uint64_t* alpha, const uint64_t* beta,
                                                const uint64_t* g1_gen, const uint64_t* g2_gen, uint64_t n_tau_g1, uint64_t n_other,
                                                const g16_srs_view* out);

}  // namespace g16
