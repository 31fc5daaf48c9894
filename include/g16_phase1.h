/* C ABI of libg16_phase1.so: phase 1 of a setup ceremony (powers of tau) over the contexts and views of g16_mi355x.h.
 *
 * A companion of libg16_mi355x.so and libg16_ceremony.so (it links against both and shares their contexts; their kernel inventories
 * are pinned by their resource tests).  It holds two kernels of its own, in four and two instantiations: the batch scalar
 * multiplication with one scalar per point, and the powers s tau^i that feed it. */
#ifndef G16_PHASE1_H
#define G16_PHASE1_H
#include "g16_ceremony.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the unit: out[i] = scalars[i] * points[i] ----
 * points: n affine points of G1 (g2 = 0) or G2 (g2 = 1), Montgomery limbs, host memory, as everywhere in this ABI; scalars: n x 4
 * words, Fr in Montgomery form (as `delta` of g16_params_apply_delta); out: n affine points, may alias points.  n = 0 is a no-op.
 * The result is exact for every scalar in [0, r) and every finite or identity input whose coordinates are below the modulus --
 * including points outside the prime-order subgroup and points off the curve (the a = 0 formulas never read b): NO on-curve or
 * membership test is made here, that is the caller's business.  A multi-device context runs on its first device.  Points go
 * through the device in chunks (G16_PHASE1_CHUNK points, read at every call; default 2^17). */
int g16_batch_scalar_mul(g16_ctx* ctx, int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out);
/* CPU only: plain double-and-add over the standard arithmetic -- deliberately a different algorithm from the device kernel */
int g16_host_batch_scalar_mul(int curve, int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out);
/* CPU only: the DEVICE kernel's task (signed 4-bit window, 30-bit lazy arithmetic, selections, the slow path) run lane by lane on the
 * host, a lane pair emulated by its two components -- what the `not gpu` tests hold against the big-integer model */
int g16_host_batch_scalar_mul_windowed(int curve, int g2, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t* out);

/* ---- a phase-1 contribution ----
 * In place over the WHOLE arrays of the view, whatever their lengths, with the contributor's secrets tau', alpha', beta' (Fr,
 * Montgomery form):
 *   tau_g1[i] <- tau'^i (.)   tau_g2[i] <- tau'^i (.)   alpha_tau_g1[i] <- alpha' tau'^i (.)   beta_tau_g1[i] <- beta' tau'^i (.)
 *   beta_g2 <- beta' (.)
 * tau_g1[0] and tau_g2[0], the generators, are not touched.  pub receives the contributor's public record tau' g2, alpha' g2,
 * beta' g2 with g2 = tau_g2[0] (three host scalar multiplications).  A zero secret is G16_ERR_UNEXPECTED_IDENTITY with nothing
 * written.  The per-point scalars are made on the device and never leave it; their buffer and the kernel's work buffer are zeroed
 * on the stream before the call returns.  The caller's copies of the secrets are the caller's to destroy.
 * The arrays are NOT checked: contribute to an SRS that the check below, or the whole-SRS check of g16_ceremony.h, accepted. */
typedef struct {
    uint64_t* tau_g2;   /* one G2 point each, affine Montgomery limbs, host memory */
    uint64_t* alpha_g2;
    uint64_t* beta_g2;
} g16_tau_contribution;
/* stream-event times of the last g16_batch_scalar_mul / g16_srs_contribute on the context, in milliseconds, summed over the chunks */
typedef struct {
    double upload_ms, powers_ms, mul_g1_ms, mul_g2_ms, download_ms;
} g16_phase1_timings;
int g16_srs_contribute(g16_ctx* ctx, const uint64_t tau[4], const uint64_t alpha[4], const uint64_t beta[4], const g16_srs_view* inout,
                       const g16_tau_contribution* pub, g16_phase1_timings* tm /* may be NULL */);
int g16_host_srs_contribute(int curve, const uint64_t tau[4], const uint64_t alpha[4], const uint64_t beta[4], const g16_srs_view* inout,
                            const g16_tau_contribution* pub, g16_phase1_timings* tm /* may be NULL; zeroed */);
int g16_phase1_get_timings(g16_ctx* ctx, g16_phase1_timings* out);

/* ---- the check of a contribution ----
 * `after` is a well-formed SRS that descends from `before` by the contribution whose G2 images are `pub`.  The flags are those of
 * g16_srs_check run on `after` (G16_SRS_*, through libg16_ceremony.so on the GPU) plus the ones below.  `before` is read at FIVE
 * points only -- tau_g1[0], tau_g1[1], tau_g2[0], alpha_tau_g1[0], beta_tau_g1[0] -- and its lengths: it was the `after` of the
 * previous round and was checked as a whole then.  The three ratio equations are two-pair products on the host.
 * coeffs / n_coeffs / info: as g16_srs_check.  bad_array continues the SRS numbering: 5, 6, 7 are pub's tau_g2, alpha_g2, beta_g2;
 * 8 is `before`, with bad_index the position in the order listed above.
 * NOT attested: who contributed (no proofs of knowledge, no transcript hashing -- only that the chain of ratios holds); .ptau
 * files are not read or written. */
#define G16_TAU_BAD_POINT 1u     /* = G16_SRS_BAD_POINT, exclusive; also pub's points and the five points of `before` (reason 4: the identity) */
#define G16_TAU_SHAPE 64u        /* array lengths differ, or after.tau_g1[0] != before.tau_g1[0], or after.tau_g2[0] != before.tau_g2[0] (bytewise) */
#define G16_TAU_RATIO 128u       /* e(after.tau_g1[1], g2) != e(before.tau_g1[1], pub.tau_g2),  g2 = before.tau_g2[0] */
#define G16_TAU_ALPHA_RATIO 256u /* e(after.alpha_tau_g1[0], g2) != e(before.alpha_tau_g1[0], pub.alpha_g2)           */
#define G16_TAU_BETA_RATIO 512u  /* e(after.beta_tau_g1[0], g2) != e(before.beta_tau_g1[0], pub.beta_g2)              */
int g16_srs_check_contribution(g16_ctx* ctx, const g16_srs_view* before, const g16_srs_view* after, const g16_tau_contribution* pub,
                               const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info);
int g16_host_srs_check_contribution(int curve, const g16_srs_view* before, const g16_srs_view* after, const g16_tau_contribution* pub,
                                    const uint64_t* coeffs, uint64_t n_coeffs, g16_ceremony_info* info);

#ifdef __cplusplus
}
#endif
#endif
