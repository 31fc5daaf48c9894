// The host planner of the MSM (msm.hip's map): window size and count, bucket groups, segment length, chunking, the walk.  No kernels.
#include "internal.hpp"
#include "msm_common.hpp"
#include <cstdlib>
#include <cstring>

namespace g16 {

#ifndef G16_REDUCE_G
#define G16_REDUCE_G 8
#endif
static constexpr uint32_t REDUCE_G = G16_REDUCE_G;   // buckets per lane in the bucket reduction

int msm_window_override() {
    const char* e = getenv("G16_MSM_WINDOW");
    return e ? atoi(e) : 0;
}

// W for a given c: smallest W with (modulus - 1) + K < 2^(cW)
static int plan_windows(int c, int scalar_bits, const uint32_t* modulus_words, int mod_nwords, uint32_t* Kout) {
    int W = (scalar_bits + 1 + c - 1) / c;
    for (;; ++W) {
        if (c * W > 320) return -1;
        uint32_t K[MSM_SWORDS] = {0};
        for (int w = 0; w < W; ++w) {
            const int bit = w * c + c - 1;
            K[bit >> 5] |= 1u << (bit & 31);
        }
        uint32_t sum[MSM_SWORDS];
        uint64_t carry = 0;
        for (int k = 0; k < MSM_SWORDS; ++k) {
            carry += (uint64_t)K[k] + (k < mod_nwords ? modulus_words[k] : 0u);
            sum[k] = (uint32_t)carry;
            carry >>= 32;
        }
        bool ok = true;  // sum = modulus + K > (modulus - 1) + K ; require sum < 2^(cW)  (conservative by one)
        for (int bit = MSM_SWORDS * 32 - 1; bit >= c * W; --bit)
            if ((sum[bit >> 5] >> (bit & 31)) & 1) { ok = false; break; }
        if (ok) {
            if (Kout) for (int k = 0; k < 10; ++k) Kout[k] = K[k];
            return W;
        }
    }
}

int msm_plan_windows(int c, int scalar_bits, const uint32_t* modulus_words, int mod_nwords) {
    return plan_windows(c, scalar_bits, modulus_words, mod_nwords, nullptr);
}

// seconds, MI355X measurements of round 1: the bucket pass folds entries at ~4.5 G mixed adds/s; the bucket reduction is
// buckets/G lanes of (2G + ~24) dependent full additions, latency-bound (~12 us each) until the lanes exceed two waves
// per SIMD; per-group bookkeeping ~4 us
static double plan_cost(uint64_t n, int W, double buckets, int groups) {
    const double acc = (double)n * W / 4.5e9;
    const double lanes = buckets / REDUCE_G;
    const double red = (2.0 * REDUCE_G + 24.0) * 12e-6 * (lanes > 131072.0 ? lanes / 131072.0 : 1.0);
    return acc + red + 4e-6 * groups;
}

int merged_window_bits(uint64_t n, int scalar_bits, const uint32_t* modulus_words, int mod_nwords) {
    const char* e = getenv("G16_MSM_PRECOMP");
    if (e && atoi(e) == 0) return 0;
    if (n == 0 || n > MSM_MERGED_MAX_N) return 0;
    const char* f = getenv("G16_MSM_PRECOMP_WINDOW");
    int c = f ? atoi(f) : 0;
    if (c <= 0) {
        double best = 1e300;
        for (int cc = MSM_MERGED_MIN_C; cc <= MSM_MERGED_MAX_C; ++cc) {
            const int W = plan_windows(cc, scalar_bits, modulus_words, mod_nwords, nullptr);
            if (W < 0 || W > 32) continue;
            const double buckets = (double)(1u << (cc - 1));
            const int groups = cc > 16 ? 1 << (cc - 16) : 1;
            // the class filter of the merged counting sort re-reads the digit planes once per class
            const double t = plan_cost(n, W, buckets, groups) + (double)n * W * groups * 3.0 / 1.5e12;
            if (t < best) { best = t; c = cc; }
        }
    }
    if (c < MSM_MERGED_MIN_C) c = MSM_MERGED_MIN_C;
    if (c > MSM_MERGED_MAX_C) c = MSM_MERGED_MAX_C;
    const int W = plan_windows(c, scalar_bits, modulus_words, mod_nwords, nullptr);
    return (W < 0 || W > 32) ? 0 : c;
}

int make_msm_plan(uint64_t n, int scalar_bits, const uint32_t* modulus_words, int mod_nwords, int merged_c, MsmPlan* plan, int shard_n,
                  int shard_r) {
    if (shard_n < 1 || shard_n > 64 || shard_r < 0 || shard_r >= shard_n || (shard_n > 1 && merged_c <= 0)) return G16_ERR_INTERNAL;
    int c = merged_c;
    if (c <= 0) {
        c = msm_window_override();
        if (c <= 0) {
            double best = 1e300;
            for (int cc = 4; cc <= 16; ++cc) {
                const int W = plan_windows(cc, scalar_bits, modulus_words, mod_nwords, nullptr);
                if (W < 0) continue;
                const double t = plan_cost(n, W, (double)W * (1u << (cc - 1)), W);
                if (t < best) { best = t; c = cc; }
            }
        }
        if (c < 3) c = 3;
        if (c > 16) c = 16;
    } else if (c < MSM_MERGED_MIN_C || c > MSM_MERGED_MAX_C || n > MSM_MERGED_MAX_N) {
        return G16_ERR_INTERNAL;
    }
    const int W = plan_windows(c, scalar_bits, modulus_words, mod_nwords, plan->K);
    if (W < 0 || (merged_c > 0 && W > 32)) return G16_ERR_INTERNAL;
    plan->c = c;
    plan->W = W;
    plan->merged = merged_c > 0;
    plan->shard_n = shard_n;
    plan->shard_r = shard_r;
    if (plan->merged) {
        // classes of B <= 2^15 buckets (what the LDS histogram holds) over the rank's buckets: all 2^(c-1) of them, or -- bucket-space
        // shard -- the ceil(2^(c-1) / shard_n) local ones (bucket shard_n k + shard_r has local index k)
        const uint32_t all = 1u << (c - 1), local = (all + (uint32_t)shard_n - 1) / (uint32_t)shard_n;
        uint32_t B = 1;
        while (B < local && B < (1u << 15)) B <<= 1;
        plan->B = B;
        plan->groups = (int)((local + B - 1) / B);
    } else {
        plan->B = 1u << (c - 1);
        plan->groups = W;
    }
    // buckets per lane of the bucket reduction: 8.  16 halves the window level's tree sums but doubles the bucket level's chain;
    // measured at 2^22 on one box (round 3, tools/ab_reduce_g.sh): 8: 77.50 / 78.11 ms, 16: 78.27 / 77.81 ms, 32: 80.56 ms -- no
    // gain, so 8 stays.  G16_MSM_REDUCE_G forces 4 / 8 / 16 / 32 (tests, A/B).
    plan->G = REDUCE_G;
    if (const char* e = getenv("G16_MSM_REDUCE_G")) {
        const int v = atoi(e);
        if (v == 4 || v == 8 || v == 16 || v == 32) plan->G = (uint32_t)v;
    }
    const uint64_t all_entries = n * (uint64_t)W / (uint64_t)shard_n;   // EXPECTED entries of this rank (uniform digits); buffers
                                                                          // are sized for the worst case in sort_scalars
    // batched-affine levels: they pay when buckets are long (each level halves a bucket's entries at ~0.6 of the XYZZ cost
    // per addition, but a lane needs >= ~16 pairs to amortise its inversion and the chip >= ~2 k waves to stay busy)
    plan->affine_levels = 0;
    {
        const uint64_t mean_load = all_entries / plan->buckets();
        // Measured (profiles/r02_affine_v1_kernel_stats.csv, 2^22, BLS12-381): the levels LOSE on this GPU -- level 0 gathers
        // every operand twice and spills a prefix product per pair (~750 B of mostly random HBM traffic per addition against
        // ~137 B for the XYZZ walk), 8.0 ms for the 27 M additions that cost the XYZZ pass 6.3 ms -- so the default is 0 and the
        // path stays as a measured, tested experiment.
        (void)mean_load;
        int R = 0;
        if (const char* e = getenv("G16_MSM_AFFINE_LEVELS")) {   // 0 disables, 1..4 forces (tests run it at tiny sizes)
            const int v = atoi(e);
            if (v >= 0 && v <= 4) R = v;
        }
        if (all_entries + (uint64_t)plan->buckets() * ((1u << R) - 1u) >= ((uint64_t)1 << 32)) R = 0;
        if (shard_n > 1) R = 0;   // (an experiment that is off by default: not carried into the bucket-space shard)
        plan->affine_levels = R;
    }
    const uint64_t entries = (all_entries >> plan->affine_levels) + (plan->affine_levels ? plan->buckets() : 0);   // what the bucket pass walks
    // Segment length of the bucket pass (entries one lane walks; the kernels take any integer >= 8): 64 entries per lane,
    // shorter for small inputs so that the pass still has >= ~4 segments per lane slot of the chip (256 CUs x 4 SIMDs x 2 waves x 64
    // lanes).  Measured at 2^22 (profiles/r03_ab_segment_length.txt, one box): 60 and 64 tie, 70 / 84 +0.8 %, 104 +1.2 %, 139 +3 %;
    // for an 8-way shard 16 and 19 tie, 28 +2 %, 56 (ONE full round of the chip) +6 %.  Lanes do not take equal time (a lane that
    // crosses more bucket boundaries flushes more partial sums), workgroups are re-dispatched one by one as others retire, so many
    // short segments balance better than few long ones, and "fill whole rounds of the chip" -- tried in round 3 -- does not pay.
    uint32_t l = 64;
    while (l > 16 && entries / l < 4ull * 131072ull) l >>= 1;
    // ... but never much shorter than the mean bucket load: a bucket of ~mean entries then touches at most ~5 segments and
    // stays below the heavy-bucket threshold (otherwise EVERY bucket would go through the cooperative combine)
    const uint64_t mean = entries / plan->buckets() + 1;
    while (l < 128 && (uint64_t)l * 4 < mean) l <<= 1;
    if (const char* e = getenv("G16_MSM_SEGMENT")) {   // experiments: force the segment length (8 .. 4096)
        const int v = atoi(e);
        if (v >= 8 && v <= 4096) l = (uint32_t)v;
    }
    plan->Lmax = l;
    // histogram / scatter chunking: ~2048 workgroups in total, chunk a multiple of 1024 points
    uint64_t nchunks = 2048 / (uint64_t)plan->groups;
    if (nchunks < 1) nchunks = 1;
    uint64_t chunk = (n + nchunks - 1) / nchunks;
    chunk = (chunk + 1023) / 1024 * 1024;
    if (chunk < 1024) chunk = 1024;
    plan->chunk = (uint32_t)chunk;
    return G16_OK;
}

// Short scalars (the ceremony library's 128-bit coefficients; sorted by sort_digit_planes, msm_sort.hip): a per-window plan over 128
// scalar bits with the "modulus" 2^128, so the smallest W with (2^128 - 1) + K < 2^(cW) -- the carry out of bit 127 and the top
// window's range -- is the plan's business; about half the windows, digit planes, histograms and per-window reductions of an Fr plan.
int coeffs128_plan(uint64_t n, MsmPlan* plan) {
    if (n >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
    const uint32_t two128[5] = {0u, 0u, 0u, 0u, 1u};   // coefficients are < 2^128
    G16_TRY(make_msm_plan(n, 128, two128, 5, 0, plan));
    plan->affine_levels = 0;   // (the G16_MSM_AFFINE_LEVELS experiment pads bucket regions: not carried into this sort)
    // rho + K < 2^(cW) <= 2^160 must fit COEFF128_SWORDS - 1 words, and the last window's second word must be the guard at most
    if (plan->merged || plan->c > 16 || plan->c * plan->W > 32 * (COEFF128_SWORDS - 2)) return G16_ERR_INTERNAL;
    for (int k = COEFF128_SWORDS - 2; k < 10; ++k)
        if (plan->K[k]) return G16_ERR_INTERNAL;
    return G16_OK;
}

int msm_prover_walk() {
    if (const char* e = getenv("G16_MSM_WALK")) {   // A/B: force either walk
        if (!strcmp(e, "segment")) return MSM_WALK_SEGMENT;
        if (!strcmp(e, "parts")) return MSM_WALK_PARTS;
    }
    return MSM_WALK_PARTS;
}

}  // namespace g16
