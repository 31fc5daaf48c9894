/* C ABI of libg16_ceremony.so: the checks a setup ceremony needs, over the contexts and views of g16_mi355x.h.
 *
 * A companion library of libg16_mi355x.so (it links against it and shares its contexts): the prover library's kernel inventory is
 * pinned by its resource tests, and these checks are a verifier's tool, not part of the proof path.  It holds two kernels of its own
 * (the digit planes of 128-bit coefficients, the first bad point of an array); the sort, the bucket passes, the reductions, the
 * membership tests and the pairing are the prover library's. */
#ifndef G16_CEREMONY_H
#define G16_CEREMONY_H
#include "g16_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ceremony checks: is an SRS a sequence of powers, does a key descend from its predecessor ----
 * The derivation above trusts its input: one wrong point in tau_g1 gives a key that proves and verifies and is unsound.  These calls
 * test what can be tested without the secrets, by pairings over random linear combinations:
 *   g16_rlc_sums             the unit: lo = sum_{i<n-1} rho_i X[i], hi = sum_{i<n-1} rho_i X[i+1] for n >= 1 points of one group --
 *                            X is a geometric sequence with ratio tau iff e(lo, tau G2) == e(hi, G2), up to 2^-128;
 *   g16_srs_check            every array of an SRS against tau_g2[1] (and tau_g2 against tau_g1[1]), beta_g2 against beta_tau_g1[0];
 *   g16_params_check_delta   `after` is `before` with more delta multiplied in: the fixed part bytewise, the deltas and the l / h
 *                            queries by the ratio after.delta / before.delta.
 * Coefficients as in g16_verify_aggregate: `coeffs` is n x 2 little-endian words (128 bits each), an explicit zero coefficient is
 * G16_ERR_BAD_ARG, coeffs == NULL draws from getrandom(2) and redraws zeros; explicit coefficients make a call deterministic and
 * must be fixed AFTER the data they test.  One coefficient vector serves every array of a call (each equation is sound on its own);
 * a shorter array uses the prefix.  Contract: with every point in its prime-order subgroup -- which the calls establish first, on
 * the same uploaded copies (flag BAD_POINT) -- a malformed input passes any ONE equation with probability <= 2^-128 over the
 * coefficients.  Points: affine Montgomery limbs, host memory, as g16_srs_view / g16_params_view.  A multi-device context runs on
 * its first device.  NOT attested: who contributed (no proofs of knowledge, no transcript -- only that the chain of ratios holds),
 * .ptau / .zkey files, gamma != 1.  Phase-1 contributions are made and checked by libg16_phase1.so (g16_phase1.h), on top of
 * g16_srs_check. */
#define G16_SRS_BAD_POINT 1u /* exclusive: no pairing is computed, no other flag reported */
#define G16_SRS_TAU_G1 2u    /* e(lo(tau_g1), tau_g2[1]) != e(hi(tau_g1), g2),  g2 = tau_g2[0]             */
#define G16_SRS_TAU_G2 4u    /* e(tau_g1[1], lo(tau_g2)) != e(g1, hi(tau_g2)),  g1 = tau_g1[0]             */
#define G16_SRS_ALPHA 8u     /* e(lo(alpha_tau_g1), tau_g2[1]) != e(hi(alpha_tau_g1), g2); vacuous for one point */
#define G16_SRS_BETA 16u     /* the same for beta_tau_g1                                                    */
#define G16_SRS_BETA_G2 32u  /* e(beta_tau_g1[0], g2) != e(g1, beta_g2)                                     */
#define G16_KEY_BAD_POINT 1u  /* exclusive, over after's delta_g1, delta_g2, l_query, h_query (arrays 0..3); l / h may be the identity */
#define G16_KEY_FIXED_PART 2u /* alpha_g1, beta_g1, beta_g2, gamma_g2, gamma_abc_g1, a_query, b_g1_query, b_g2_query (arrays 0..7) differ */
#define G16_KEY_DELTA 4u      /* e(after.delta_g1, before.delta_g2) != e(before.delta_g1, after.delta_g2)  */
#define G16_KEY_L 8u          /* e(sum rho after.l, after.delta_g2) != e(sum rho before.l, before.delta_g2) */
#define G16_KEY_H 16u         /* the same for h_query                                                       */
typedef struct {
    uint32_t flags;      /* 0: every check holds; else the OR of the flags above                                              */
    uint32_t bad_array;  /* BAD_POINT: the array in the view's field order (SRS: tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1,     */
                         /* beta_g2); FIXED_PART: the first differing field in the order listed above                         */
    uint64_t bad_index;  /* the first such point of that array (deterministic: the smallest index)                            */
    uint32_t bad_reason; /* BAD_POINT: 2 off its curve, 3 outside the prime-order subgroup, 4 the identity; else 0            */
    uint32_t reserved;
} g16_ceremony_info;
/* out_lo, out_hi: one affine point each; n = 1 gives two identities.  One upload, one sort of the n - 1 coefficients (a plan over
 * 128 scalar bits), two bucket passes over that sort in one launch, one batch of reductions.  g16_get_timings afterwards reports the
 * plan's window_bits and windows. */
int g16_rlc_sums(g16_ctx* ctx, int g2, const uint64_t* points, uint64_t n, const uint64_t* coeffs, uint64_t* out_lo, uint64_t* out_hi);
/* the plan n_coeffs coefficients are sorted with (no GPU needed): out[0] = window bits c, out[1] = windows W, out[2] = coefficients per
 * histogram / scatter workgroup, out[3] = entries one bucket-pass lane walks */
int g16_rlc_plan(uint64_t n_coeffs, uint32_t out[4]);
/* The whole arrays of the view are tested, not a prefix.  Needs n_tau_g1 >= 2, n_tau_g2 >= 2, n_alpha_beta >= 1 and, for explicit
 * coefficients, n_coeffs >= max(n_tau_g1, n_tau_g2, n_alpha_beta) - 1: else G16_ERR_BAD_LENGTH with g16_last_error naming the array. */
int g16_srs_check(g16_ctx* ctx, const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info);
/* before / after: two keys of one shape in host memory (G16_PARAMS_DEVICE_PTRS is refused); n_l / n_h: points of l_query / h_query.
 * Explicit coefficients need n_coeffs >= max(n_l, n_h) (here the sums run over ALL points: sum_{i<n} rho_i X[i]). */
int g16_params_check_delta(g16_ctx* ctx, const g16_params_view* before, const g16_params_view* after, uint64_t n_vars, uint64_t n_inputs,
                           uint64_t n_l, uint64_t n_h, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info);
/* stream-event times of the last of the three calls above on this context, in milliseconds (pairings: the wall clock of the two-pair products, which run on the host) */
typedef struct {
    double upload_ms, membership_ms, sort_ms, passes_ms, reductions_ms, pairings_ms;
} g16_ceremony_timings;
int g16_ceremony_get_timings(g16_ctx* ctx, g16_ceremony_timings* out);
/* CPU only: plain scalar multiplications and additions, the host membership tests and the host pairing (the `not gpu` tests) */
int g16_host_rlc_sums(int curve, int g2, const uint64_t* points, uint64_t n, const uint64_t* coeffs, uint64_t* out_lo, uint64_t* out_hi);
int g16_host_srs_check(int curve, const g16_srs_view* srs, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info);
int g16_host_params_check_delta(int curve, const g16_params_view* before, const g16_params_view* after, uint64_t n_vars, uint64_t n_inputs,
                                uint64_t n_l, uint64_t n_h, const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info);

#ifdef __cplusplus
}
#endif
#endif
