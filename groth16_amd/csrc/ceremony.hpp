// libg16_ceremony.so (ceremony.hip, include/g16_ceremony.h) over the internals of libg16_mi355x.so: what the companion library takes
// from a context.  Everything else it uses -- the plan and sort of short scalars, the bucket passes and reductions, convert_bases,
// the membership launches, agg_coeffs -- is declared in internal.hpp / verify_common.hpp and defined in the prover library.
#pragma once
#include "internal.hpp"

namespace g16 {

// the first device's stream and arena of a context; api.hip fills it, makes the device current and resets the arena first
struct CeremonyEnv {
    hipStream_t st;
    Arena* arena;
    double* stage_ms;               // [6]: upload, membership, sort, passes, reductions, pairings of the last call (kept in the context)
    double *window_bits, *windows;  // the coefficient plan's c and W (g16_timings)
};
int ceremony_enter(g16_ctx* ctx, CeremonyEnv* env, int* curve);
const double* ceremony_stage_ms(const g16_ctx* ctx);
double* phase1_stage_ms(g16_ctx* ctx);      // [5]: the stage times of libg16_phase1.so's last call (kept in the context)
double* keycheck_stage_ms(g16_ctx* ctx);    // [10]: g16_keycheck_timings of libg16_keycheck.so's last call (kept in the context)
double* lagrange_stage_ms(g16_ctx* ctx);    // [6]: g16_lagrange_timings of libg16_lagrange.so's last call (kept in the context)
void set_last_error_text(const char* text);   // what g16_last_error returns next on this thread

}  // namespace g16
