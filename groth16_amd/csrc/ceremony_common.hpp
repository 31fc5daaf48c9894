// What the three companion libraries share: ceremony.hip (libg16_ceremony.so), phase1.hip (libg16_phase1.so) and keycheck.hip
// (libg16_keycheck.so), and only they include it -- ceremony.hpp, which api.hip sees, does not.  Host code only, no kernel: the stage
// timers and the wait every exit makes, uploads into the call's arena, the two groups of a curve, a membership flag as the reason of
// g16_ceremony_info, the record of a call's first bad point, the two-pair equation, the refusals with a text, the checks of a
// g16_srs_view and a context's stage times as a library's timings struct.
#pragma once
#include "ceremony.hpp"
#include "../../include/g16_ceremony.h"
#include "subgroup.hpp"
#include "verify_common.hpp"
#include <deque>

namespace g16 {

// the event timers of one stage of one call.  add() hands out a pointer that the callee keeps (msm_bucket_pass*); a deque never moves
// its elements, so the pointer stays valid however many timers follow
struct Timers {
    std::deque<EventTimer> v;
    ~Timers() { for (auto& t : v) t.destroy(); }
    EventTimer* add() { v.emplace_back(); return &v.back(); }
    double total() { double s = 0; for (auto& t : v) s += t.ms(); return s; }
};
// kernels in flight read arena memory that the next call reuses and write host vectors of this one: every exit waits
struct StreamWait {
    hipStream_t s;
    ~StreamWait() { (void)hipStreamSynchronize(s); }
};
inline double wall_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// n elements of host memory into the call's arena, on its stream (n = 0: an allocation of one element, no copy)
template <class T>
int upload(const CeremonyEnv& env, const void* host, uint64_t n, T** out) {
    G16_TRY(env.arena->alloc_n(n ? n : 1, out));
    if (n) G16_HIP_TRY(hipMemcpyAsync(*out, host, n * sizeof(T), hipMemcpyHostToDevice, env.st));
    return G16_OK;
}

// G1 (G2 = 0) or G2 (G2 = 1) of a curve
template <class C, int G2> struct Grp;
template <class C>
struct Grp<C, 0> {
    typedef typename C::Fq F;
    typedef Affine<F> A;
    static constexpr uint32_t WORDS = C::Fq::N;   // 64-bit words of an affine point
    static uint8_t flag(const A& p) { return Subgroup<C>::g1_flag(p); }
};
template <class C>
struct Grp<C, 1> {
    typedef typename C::Fq2 F;
    typedef Affine<F> A;
    static constexpr uint32_t WORDS = 2 * C::Fq::N;
    static uint8_t flag(const A& p) { return Subgroup<C>::g2_flag(p); }
};

// a membership flag (1 in the subgroup, 2 off the curve, 0 outside the subgroup) as the bad_reason of g16_ceremony_info; 0: a good point
inline uint32_t flag_reason(uint8_t flag, bool allow_identity, bool is_identity = false) {
    return flag == 2 ? 2u : flag == 0 ? 3u : (!allow_identity && is_identity) ? 4u : 0u;
}
template <class C, int G2>
uint32_t point_reason(const typename Grp<C, G2>::A& p, bool allow_identity) {
    return flag_reason(Grp<C, G2>::flag(p), allow_identity, p.is_identity());
}

// The first bad point of a call as one word: array << 48 | index << 8 | reason (index < 2^31), so that the smaller word is the point
// that comes first in the call's order; BAD_NONE: every point passed.  ceremony_first_bad_kernel (ceremony.hip) mirrors this layout on
// the device, where it takes the atomic minimum of such words: change the two together.
constexpr unsigned long long BAD_NONE = ~0ull;
inline unsigned long long bad_key(uint32_t array, uint64_t index, uint32_t reason) {
    return ((unsigned long long)array << 48) | ((unsigned long long)index << 8) | reason;
}
inline void decode_bad(unsigned long long key, uint32_t flag, g16_ceremony_info* info) {
    info->flags = flag;
    info->bad_array = (uint32_t)(key >> 48);
    info->bad_index = (key >> 8) & 0xffffffffffull;
    info->bad_reason = (uint32_t)(key & 0xffu);
}

// e(a, b) == e(c, d), as the two-pair product e(a, b) e(-c, d) compared with 1.  On the host templates for the device forms too, as
// the once-per-batch tail of verify_aggregate.hip: a lone GPU lane runs this chain several times slower than one host thread, and a
// call has a handful of them whatever the size of its arrays
template <class C>
int pairs_equal(const typename C::G1A& a, const typename C::G2A& b, const typename C::G1A& c, const typename C::G2A& d, bool* equal) {
    typedef Pairing<C> PP;
    const typename C::G1A g1s[2] = {a, c.neg()};
    const typename C::G2A g2s[2] = {b, d};
    typename PP::F12 e;
    *equal = host_pairing_product<C>(reinterpret_cast<const uint64_t*>(g1s), reinterpret_cast<const uint64_t*>(g2s), 2, e) &&
             PP::equal(e, PP::F12::one());
    return G16_OK;
}

// status, with fmt (its arguments: name, a, b, c) as the text g16_last_error returns next
inline int refuse(int status, const char* fmt, unsigned long long a, unsigned long long b, unsigned long long c, const char* name = "") {
    char buf[256];
    snprintf(buf, sizeof(buf), fmt, name, a, b, c);
    set_last_error_text(buf);
    return status;
}

// ---- a g16_srs_view -----------------------------------------------------------------------------------------------------------------
inline bool srs_view_ok(const g16_srs_view* s) { return s->tau_g1 && s->tau_g2 && s->alpha_tau_g1 && s->beta_tau_g1 && s->beta_g2; }

// One array of a view against what the call needs of it.  srs_lengths refuses the first array of the caller's table that holds fewer
// points than it needs with the text too_short (refuse's arguments: name, have, need, c) and, where too_long is given, one that holds
// 2^31 points or more with that text (name), in the table's order
struct SrsArray {
    const char* name;
    uint64_t have, need;
};
template <size_t N>
int srs_lengths(const SrsArray (&arr)[N], const char* too_short, unsigned long long c, const char* too_long = nullptr) {
    for (const SrsArray& a : arr) {
        if (a.have < a.need) return refuse(G16_ERR_BAD_LENGTH, too_short, a.have, a.need, c, a.name);
        if (too_long && a.have >= ((uint64_t)1 << 31)) return refuse(G16_ERR_BAD_LENGTH, too_long, 0, 0, 0, a.name);
    }
    return G16_OK;
}

// ---- the stage times of a library's last call: N doubles in the context (ceremony.hpp), read and written as its timings struct T ----
template <class T, int N>
struct StageTimes {
    static_assert(sizeof(T) == N * sizeof(double), "the context keeps the stage times as N doubles");
    static T* of(double* ms) { return reinterpret_cast<T*>(ms); }
    // the body of g16_*_get_timings; ms: null for no context
    static int get(const double* ms, T* out) {
        if (!ms || !out) return G16_ERR_BAD_ARG;
        memcpy(out, ms, sizeof(T));
        return G16_OK;
    }
};

}  // namespace g16
