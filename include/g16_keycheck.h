/* C ABI of libg16_keycheck.so: is a proving key THE key of a circuit over an SRS -- decided without deriving the key again.
 *
 * A companion of libg16_mi355x.so, libg16_ceremony.so and libg16_phase1.so (it links against them and shares their contexts; their
 * kernel inventories are pinned by their resource tests).  It holds four kernels of its own, each for both scalar fields: the
 * 128-bit coefficients as Montgomery Fr, the row walk over A, B and C with split sums, the odd-position scatter of the Circom h
 * vector and the sum of two vectors.  The scalar transforms, the digit sort, the bucket passes, the reductions,
 * convert_bases, the membership launches and the pairing are the prover library's. */
#ifndef G16_KEYCHECK_H_INCLUDED
#define G16_KEYCHECK_H_INCLUDED
#include "g16_ceremony.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the check ----
 * Every query of a key derived by g16_generate_parameters_srs is a linear image of SRS points under the circuit's matrices and the
 * inverse n-point transform, whose matrix (n^-1 w^(-ik)) is symmetric.  So a random linear combination of a query equals ONE MSM
 * over the SRS itself whose scalars come from a sparse mat-vec and a scalar transform of the coefficients: with A~ = A plus the
 * instance-copy rows, T_k = tau_g1[k], w_M(x) = ifft_n(M x) (natural order, n^-1 included) and rho a vector over the variables,
 *     sum_j rho_j a_query[j] = sum_{k<n} w_A~(rho)[k] T_k.
 * rho_in is rho on j < num_inputs and 0 elsewhere, rho_aux the rest; g1 = tau_g1[0], g2 = tau_g2[0]; d1, d2 the key's deltas.
 *
 *   flag        equation
 *   BAD_POINT   (exclusive) every point of a_query, b_g1_query, b_g2_query, gamma_abc_g1, l_query, h_query, delta_g1, delta_g2
 *               (arrays 0..7 in this order) is on its curve and in its subgroup; the identity is allowed in the six arrays and
 *               refused for the two deltas.  bad_array / bad_index / bad_reason as in g16_ceremony_info: the first array with a
 *               bad point, its smallest index.
 *   FIXED       alpha_g1 = alpha_tau_g1[0], beta_g1 = beta_tau_g1[0], beta_g2 = srs.beta_g2, gamma_g2 = g2, bytewise (bad_array:
 *               the first of the four that differs)
 *   DELTA       e(d1, g2) = e(g1, d2)
 *   A           sum rho_j a_query[j] = MSM(tau_g1[0..n), w_A~(rho))                       (point equality, no pairing)
 *   B_G1, B_G2  the same with B (no instance rows), over tau_g1 and over tau_g2
 *   GAMMA_ABC   sum_{j<ni} rho_j gamma_abc_g1[j] = MSM(beta_tau_g1, w_A~(rho_in)) + MSM(alpha_tau_g1, w_B(rho_in)) + MSM(tau_g1, w_C(rho_in))
 *   L           e(sum_{j>=ni} rho_j l_query[j - ni], d2) = e(the same three-MSM sum with rho_aux, g2)
 *   H           Libsnark: e(sum_{i<n-1} rho_i h[i], d2) = e(sum rho_i tau_g1[i + n] - sum rho_i tau_g1[i], g2)
 *               Circom:   e(sum_{j<n} rho_j h[j], d2) = e(MSM(tau_g1[0..2n-1), ifft_2n(e)[0..2n-1)), g2),  e[2j+1] = rho_j, e[even] = 0
 *
 * A key with any number of delta contributions passes, and so does the delta = 1 key fresh from g16_generate_parameters_srs.
 * PRECONDITION: the SRS has passed g16_srs_check.  The soundness argument needs the SRS points in their subgroups and the arrays
 * to be the powers they claim; this call does not test them.  Contract: with every point of the key in its prime-order subgroup --
 * established here first (BAD_POINT) -- a key that differs from the true key in any point passes the equation of that point with
 * probability <= 2^-128 over rho.  gamma = 1, as everywhere in the SRS path.  NOT attested: who contributed, gamma != 1; no file
 * formats are read or written.
 * Coefficients: as g16_srs_check; explicit ones need n_coeffs >= max(num_variables, h length).  rho_j belongs to variable j, and
 * the h equations reuse the prefix.  Lengths: the SRS arrays as g16_generate_parameters_srs needs them (G16_ERR_BAD_LENGTH); a
 * domain beyond the two-adicity is G16_ERR_DEGREE_TOO_LARGE (Circom: the bound is on 2n).  The key is a HOST view
 * (G16_PARAMS_DEVICE_PTRS is refused) with num_variables points in a / b_g1 / b_g2, num_inputs in gamma_abc_g1, the rest in
 * l_query and the reduction's h length (g16_h_query_len) in h_query.  A multi-device context runs on its first device. */
#define G16_KEYCHECK_BAD_POINT 1u
#define G16_KEYCHECK_FIXED 2u
#define G16_KEYCHECK_DELTA 4u
#define G16_KEYCHECK_A 8u
#define G16_KEYCHECK_B_G1 16u
#define G16_KEYCHECK_B_G2 32u
#define G16_KEYCHECK_GAMMA_ABC 64u
#define G16_KEYCHECK_L 128u
#define G16_KEYCHECK_H 256u
int g16_params_check_derivation(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables,
                                int qap, const g16_srs_view* srs, const g16_params_view* key, const uint64_t* coeffs, uint64_t n_coeffs,
                                g16_ceremony_info* info);

/* ---- the unit: the SRS side alone ----
 * The right-hand sides of A, B_G1, B_G2, GAMMA_ABC, L and H before any pairing: one affine point each (b_g2 in G2), host memory.
 * Deterministic for explicit coefficients, which this call requires (coeffs == NULL is G16_ERR_BAD_ARG). */
typedef struct {
    uint64_t* a;
    uint64_t* b_g1;
    uint64_t* b_g2;
    uint64_t* gamma_abc;
    uint64_t* l;
    uint64_t* h;
} g16_key_fold;
int g16_key_fold_from_srs(g16_ctx* ctx, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables, int qap,
                          const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, const g16_key_fold* out);

/* stream-event times of the last of the two calls above on this context, in milliseconds (pairings: the wall clock of the two-pair
 * products, which run on the host; transforms include building the domain tables), and the plan the full-size scalars were sorted
 * with: raw bases, no window tables, one window per group (window_bits c, windows W) */
typedef struct {
    double upload_ms, membership_ms, rows_ms, transforms_ms, sorts_ms, passes_ms, reductions_ms, pairings_ms, window_bits, windows;
} g16_keycheck_timings;
int g16_keycheck_get_timings(g16_ctx* ctx, g16_keycheck_timings* out);

/* CPU only: the same row walk, radix-2 transforms, bucket-method sums, the host membership tests and the host pairing (the `not gpu`
 * tests and the reference of the GPU tests) */
int g16_host_params_check_derivation(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints,
                                     uint64_t num_variables, int qap, const g16_srs_view* srs, const g16_params_view* key,
                                     const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info);
int g16_host_key_fold_from_srs(int curve, const g16_csr_view abc[3], uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables,
                               int qap, const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, const g16_key_fold* out);

#ifdef __cplusplus
}
#endif
#endif
