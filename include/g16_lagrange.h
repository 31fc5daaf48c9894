/* C ABI of libg16_lagrange.so: the Lagrange form of a powers-of-tau SRS, made once per domain, and a circuit's proving key derived
 * from it (what snarkjs calls `powersoftau prepare phase2`), over the contexts and views of g16_mi355x.h.
 *
 * A companion of libg16_mi355x.so, libg16_ceremony.so and libg16_phase1.so (it links against them and shares their contexts; their
 * kernel inventories are pinned by their resource tests).  It holds three kernels of its own, in four instantiations each (G1 and
 * G2 of both curves): the butterfly's sum and difference, the twiddle multiplication on phase 1's windowed task, and the bit
 * reversal. */
#ifndef G16_LAGRANGE_H
#define G16_LAGRANGE_H
#include "g16_phase1.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the unit: the transform of g16_group_ntt on the windowed scalar multiplication ----
 * points: n = 2^log_n affine points of G1 (g2 = 0) or G2 (g2 = 1), Montgomery limbs, host memory, natural order in and out; out may
 * alias points.  inverse: the inverse root and the factor n^-1.  The result is bit-equal to g16_group_ntt's for every array of
 * points ON THE CURVE (identities and points outside the prime-order subgroup included).  A stage runs in chunks of at most
 * G16_LAGRANGE_CHUNK butterflies (read at every call; default 2^17, minimum 1).  A multi-device context runs on its first device. */
int g16_group_ntt_windowed(g16_ctx* ctx, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out);
/* CPU only: the DEVICE kernels' tasks run butterfly by butterfly on the host, a lane pair emulated by its two components */
int g16_host_group_ntt_windowed(int curve, int g2, const uint64_t* points, int log_n, int inverse, uint64_t* out);

/* ---- the Lagrange form of an SRS for a domain of n = 2^log_n points and one reduction ----
 * Everything of the SRS that g16_generate_parameters_srs reads, with the circuit-independent work done: host memory, affine
 * Montgomery limbs.  The caller owns the arrays. */
typedef struct {
    uint64_t* u_g1;        /* n points: L_i(tau) G1, the inverse transform of tau_g1[0 .. n) */
    uint64_t* alpha_u_g1;  /* n points: the same of alpha_tau_g1 */
    uint64_t* beta_u_g1;   /* n points: the same of beta_tau_g1 */
    uint64_t* u_g2;        /* n points: the same of tau_g2 */
    uint64_t* h_g1;        /* the delta = 1 h_query of the reduction: n - 1 points (Libsnark) or n (Circom) */
    uint64_t* tau_g1_0;    /* one point each: tau_g1[0], alpha_tau_g1[0], beta_tau_g1[0], tau_g2[0], beta_g2 */
    uint64_t* alpha_g1_0;
    uint64_t* beta_g1_0;
    uint64_t* tau_g2_0;
    uint64_t* beta_g2;
    int32_t log_n;
    int32_t qap;           /* g16_qap */
} g16_lagrange_srs_view;

/* Fills the arrays of `out` and records log_n and qap in it.  The SRS lengths are checked as g16_generate_parameters_srs checks them
 * (tau_g1: 2n - 1 points, the others n; a longer SRS is fine); the SRS itself is NOT checked (g16_srs_check does that). */
int g16_srs_lagrange(g16_ctx* ctx, const g16_srs_view* srs, int log_n, int qap, g16_lagrange_srs_view* out);
int g16_host_srs_lagrange(int curve, const g16_srs_view* srs, int log_n, int qap, g16_lagrange_srs_view* out);

/* The key that g16_generate_parameters_srs derives for the reduction lagrange->qap, byte for byte, from the Lagrange form of its SRS:
 * the sparse products and the copies only.  A view whose log_n is not the circuit's domain is G16_ERR_BAD_LENGTH, a qap that is no g16_qap
 * G16_ERR_BAD_ARG; g16_last_error names the mismatch.  A Lagrange form that did not come from g16_srs_lagrange needs no check of
 * its own: the derived key fails g16_params_check_derivation against the raw SRS. */
int g16_generate_parameters_lagrange(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                     uint64_t num_variables, const g16_lagrange_srs_view* lagrange, const g16_params_view* out);
int g16_host_generate_parameters_lagrange(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                          uint64_t num_variables, const g16_lagrange_srs_view* lagrange, const g16_params_view* out);

/* stream-event milliseconds of the last g16_srs_lagrange (the four arrays and the h basis, uploads and downloads included) and of
 * the last g16_generate_parameters_lagrange (products, as g16_srs_timings.products_ms) on the context; g16_group_ntt_windowed
 * reports its one transform as u_g1_ms (g2 = 0) or u_g2_ms (g2 = 1) */
typedef struct {
    double u_g1_ms, alpha_u_g1_ms, beta_u_g1_ms, u_g2_ms, h_ms, products_ms;
} g16_lagrange_timings;
int g16_lagrange_get_timings(g16_ctx* ctx, g16_lagrange_timings* out);

#ifdef __cplusplus
}
#endif
#endif
