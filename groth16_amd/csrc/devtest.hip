// The field lab: single operations of the 30-bit lazy arithmetic (fp30.hpp) on raw limbs, one tuple per lane on the device
// (g16_dev_fp30_op) and the same functor compiled for the host (g16_host_fp30_op).  Test hooks like hosttest.hip: not on a proof's
// path.  On the device the product forms go through the public Fp30 members, i.e. through the generated assembly blocks of
// fips_asm_gen.hpp; the lane-pair forms run with one Fq2 value per adjacent lane pair and their DPP moves live.  The host has no
// lanes: its lane-pair forms call the pair's pure per-lane routines once with hi = false and once with hi = true.
// The accumulator forms put a lazy Acc30 through a chain of mixed additions (G1, G2 in one lane, G2 on the lane pair: device only).
// The parked forms do the same with the bucket pass's own accumulator: AccParked over LdsAccStore in the kernel's LDS layout, signed
// additions from packed y, gather() and to_packed as the flush does (G1; G2 on the lane pair: device only).  The host twin of the G1
// form parks in ParkedArrayStore.
// The inversion forms run the division-step inverse (ModInv30, batch_inverse, and pair_inverse on the lane pair with its DPP swap live),
// the doubling forms jac30_double of the window-table builder, the affine forms one pair of the batched-affine tree (classify, the
// inverse of its denominator, finish); the lane-pair doubling and affine forms are device only.
// Kernel names start with devlab_: no resource budget applies to them.
#include "internal.hpp"
#include "fp30.hpp"
#include "acc_store.hpp"
#include "batch_affine.hpp"
#include "window_tables.hpp"
#include <type_traits>
#include <vector>

using namespace g16;

namespace g16 {
int ctx_devices(const g16_ctx* ctx, int* curve, std::vector<int>& devs, std::vector<hipStream_t>& streams);   // api.hip
}

namespace {

// operand / output slots of a form (a slot is NL 32-bit words); false for an unknown form.  include/g16_mi355x.h lists the forms.
constexpr bool lab_slots(int form, int* nin, int* nout) {
    int i = 0, o = 1;
    switch (form) {
        case 0: i = 2; break;
        case 1: i = 1; break;
        case 2: i = 4; break;
        case 3: i = 8; break;
        case 4: case 6: case 8: i = 3; break;
        case 5: case 7: case 9: i = 5; break;
        case 10: i = 4; break;
        case 11: i = 3; break;
        case 20: case 21: case 22: case 23: case 24: case 25: i = 2; break;
        case 26: i = 1; break;
        case 27: i = 3; break;
        case 28: i = 2; o = 2; break;
        case 30: case 31: case 32: case 33: case 34: case 35: case 36: case 37: case 38: case 39: case 40: case 41: case 42: case 43: i = 1; break;
        case 50: i = 4; o = 2; break;
        case 51: i = 2; o = 2; break;
        case 60: i = 4; o = 2; break;
        case 61: i = 2; o = 2; break;
        case 62: i = 6; o = 2; break;
        case 63: case 64: case 65: i = 8; o = 2; break;
        case 70: i = 11; o = 5; break;
        case 71: case 72: i = 21; o = 9; break;
        case 73: i = 11; o = 5; break;
        case 74: i = 21; o = 9; break;
        case 80: case 81: i = 1; break;
        case 82: i = 2; o = 2; break;
        case 83: i = 4; o = 3; break;
        case 84: i = 7; o = 6; break;
        case 85: i = 5; o = 3; break;
        case 86: i = 9; o = 5; break;
        default: return false;
    }
    *nin = i;
    *nout = o;
    return true;
}
constexpr int lab_nin(int form) { int i = 0, o = 0; lab_slots(form, &i, &o); return i; }
constexpr int lab_nout(int form) { int i = 0, o = 0; lab_slots(form, &i, &o); return o; }
constexpr bool lab_is_pair(int form) { return (form >= 60 && form < 70) || form == 72 || form == 74 || form == 82 || form == 84 || form == 86; }
constexpr bool lab_is_parked(int form) { return form == 73 || form == 74; }
// the lane pair's accumulators, doublings and affine pairs need their lanes
constexpr bool lab_device_only(int form) { return form == 72 || form == 74 || form == 84 || form == 86; }
// base fields have the fused-subtraction products, the Fq2 forms and the lane pair; scalar fields have sub_pow2
template <class P>
constexpr bool lab_has(int form) {
    constexpr bool base = FipsAsm<P>::has_sub;
    if ((form >= 4 && form <= 11) || form >= 50) return base;
    if (form == 27) return !base;
    return true;
}

template <class P> G16_HD Fp30<P> ld(const uint32_t* s, int k) {
    Fp30<P> r;
    G16_UNROLL for (int i = 0; i < Fp30<P>::NL; ++i) r.l[i] = s[k * Fp30<P>::NL + i];
    return r;
}
template <class P> G16_HD void st(uint32_t* o, int k, const Fp30<P>& v) {
    G16_UNROLL for (int i = 0; i < Fp30<P>::NL; ++i) o[k * Fp30<P>::NL + i] = v.l[i];
}
template <class P> G16_HD void st_flag(uint32_t* o, int k, bool b) {
    G16_UNROLL for (int i = 0; i < Fp30<P>::NL; ++i) o[k * Fp30<P>::NL + i] = (i == 0 && b) ? 1u : 0u;
}
// the packed form (NW 32-bit words) in a slot of NL words
template <class P> G16_HD Fp<P> ld_words(const uint32_t* s, int k) {
    Fp<P> r;
    G16_UNROLL for (int i = 0; i < P::N; ++i) r.v[i] = s[k * Fp30<P>::NL + i];
    return r;
}
template <class P> G16_HD void st_words(uint32_t* o, int k, const Fp<P>& v) {
    G16_UNROLL for (int i = 0; i < Fp30<P>::NL; ++i) o[k * Fp30<P>::NL + i] = i < P::N ? v.v[i] : 0u;
}

// The accumulator-level form: a lazy XYZZ accumulator (Acc30, register-resident) takes a chain of up to three mixed additions.
// A field element occupies C slots (C = 1 for Fq, 2 for Fq2; the lane pair reads and writes the slot of its own component `hi`):
//   in:  x y zz zzz (raw lazy limbs: x < 7.5 p, y < 3.5 p, zz, zzz < 1.8 p) | one flag slot: word 0 the accumulator is the identity,
//        word 1 the number of points, word 2 + j point j is the identity (skipped, as the bucket kernels skip it) | x y of three points
//   out: x y zz zzz as to_packed leaves them (canonical, 32-bit words) | word 0 of the last slot: the result is the identity
template <class P, class F>
struct AccLab {
    typedef Fp30<P> B;
    static constexpr int C = sizeof(F) == sizeof(B) && F::LANES_PER_TASK == 1 ? 1 : 2;
    G16_HD static F ldf(const uint32_t* in, int slot, int hi) {
        if constexpr (F::LANES_PER_TASK == 2) return F{ld<P>(in, slot + hi)};
        else if constexpr (C == 2) return F{ld<P>(in, slot), ld<P>(in, slot + 1)};
        else return ld<P>(in, slot);
    }
    G16_HD static void stf(uint32_t* out, int slot, int hi, const F& v) {
        if constexpr (F::LANES_PER_TASK == 2) st_words<P>(out, slot + hi, v.c.to_packed());
        else if constexpr (C == 2) { st_words<P>(out, slot, v.c0.to_packed()); st_words<P>(out, slot + 1, v.c1.to_packed()); }
        else st_words<P>(out, slot, v.to_packed());
    }
    G16_HD static void run(const uint32_t* in, uint32_t* out, int hi) {
        const uint32_t* flags = in + 4 * C * B::NL;
        Acc30<F> a;
        a.x = ldf(in, 0, hi); a.y = ldf(in, C, hi); a.zz = ldf(in, 2 * C, hi); a.zzz = ldf(in, 3 * C, hi);
        a.inf = flags[0] != 0;
        const int n = flags[1] > 3u ? 3 : (int)flags[1];
        for (int j = 0; j < n; ++j) {
            if (flags[2 + j] != 0) continue;
            a.add_affine(ldf(in, 4 * C + 1 + 2 * j * C, hi), ldf(in, 4 * C + 1 + (2 * j + 1) * C, hi));
        }
        if (a.inf) a.x = a.y = a.zz = a.zzz = F::zero();
        stf(out, 0, hi, a.x); stf(out, C, hi, a.y); stf(out, 2 * C, hi, a.zz); stf(out, 3 * C, hi, a.zzz);
        if (F::LANES_PER_TASK == 1 || hi == 0) st_flag<P>(out, 4 * C, a.inf);
    }
};

// The bucket pass's accumulator (bucket_accumulate30_kernel): AccParked, coordinates behind a store, the sum's sign tracked in `neg`.
// Same slots as AccLab, with the points as the window table holds them (canonical PACKED words, x and y) and more flags:
//   in:  x y zz zzz (raw lazy limbs, the coordinates AS THEY LIE: the represented point is -(x, y, zz, zzz) when neg is set) |
//        flag slot: word 0 the accumulator is the identity, word 1 the initial neg (kept as given beside an identity flag too: a
//        flush or a cancellation leaves it behind), word 2 the number of points, word 3 + j point j is the identity (skipped, as
//        the kernel skips it), word 6 + j point j is subtracted (`minus`, the signed digit's sign) | x y of three points
//   out: gather() -- what a flush hands to the reductions -- through to_packed | word 0 of the last slot: the result is the identity
template <class P, class F, class Store>
struct ParkedLab {
    typedef Fp30<P> B;
    static constexpr int C = F::LANES_PER_TASK == 2 ? 2 : 1;
    G16_HD static F ldf(const uint32_t* in, int slot, int hi) {
        if constexpr (C == 2) return F{ld<P>(in, slot + hi)};
        else return ld<P>(in, slot);
    }
    G16_HD static void stf(uint32_t* out, int slot, int hi, const F& v) {
        if constexpr (C == 2) st_words<P>(out, slot + hi, v.c.to_packed());
        else st_words<P>(out, slot, v.to_packed());
    }
    G16_HD static void run(const uint32_t* in, uint32_t* out, int hi, AccParked<F, Store>& a) {
        const uint32_t* flags = in + 4 * C * B::NL;
        a.inf = flags[0] != 0;
        a.neg = flags[1] != 0;
        if (!a.inf) {
            a.s.st(a.CX, ldf(in, 0, hi)); a.s.st(a.CY, ldf(in, C, hi)); a.s.st(a.CZZ, ldf(in, 2 * C, hi)); a.s.st(a.CZZZ, ldf(in, 3 * C, hi));
        }
        const int n = flags[2] > 3u ? 3 : (int)flags[2];
        for (int j = 0; j < n; ++j) {
            if (flags[3 + j] != 0) continue;
            const Fp<P> xw = ld_words<P>(in, 4 * C + 1 + 2 * j * C + hi), yw = ld_words<P>(in, 4 * C + 1 + (2 * j + 1) * C + hi);
            a.add_affine_packed(F{B::unpack(xw.v)}, yw, flags[6 + j] != 0);
        }
        Acc30<F> g = a.gather();
        if (g.inf) g.x = g.y = g.zz = g.zzz = F::zero();
        stf(out, 0, hi, g.x); stf(out, C, hi, g.y); stf(out, 2 * C, hi, g.zz); stf(out, 3 * C, hi, g.zzz);
        if (C == 1 || hi == 0) st_flag<P>(out, 4 * C, g.inf);
    }
};

// d times jac30_double (window_tables.hpp).  A field element occupies C slots (the lane pair reads and writes the slot of its own
// component `hi`):  in: X Y Z raw lazy limbs | word 0 of the last slot: d, clamped to 1 .. 32   out: X Y Z as the doublings left them
template <class P, class F>
struct JacLab {
    static constexpr int C = F::LANES_PER_TASK;
    G16_HD static F ldf(const uint32_t* in, int slot, int hi) { return TableLane<F>::wrap(ld<P>(in, slot + hi)); }
    G16_HD static void run(const uint32_t* in, uint32_t* out, int hi) {
        F X = ldf(in, 0, hi), Y = ldf(in, C, hi), Z = ldf(in, 2 * C, hi);
        const uint32_t dw = in[3 * C * Fp30<P>::NL];
        const int d = dw < 1u ? 1 : dw > 32u ? 32 : (int)dw;
        for (int k = 0; k < d; ++k) jac30_double(X, Y, Z);
        st<P>(out, hi, TableLane<F>::comp(X)); st<P>(out, C + hi, TableLane<F>::comp(Y)); st<P>(out, 2 * C + hi, TableLane<F>::comp(Z));
    }
};

// One pair of the batched-affine tree: classify, the inverse of the pair's own denominator, finish.  Stricter than AffineLevel::run,
// which inverts the running prefix product (an output of mul, below 1.06p): here batch_inverse gets the raw d, up to 3p per component.
//   in:  a flag slot (word 0: P is the identity, word 1: Q is) | px py qx qy canonical limbs
//   out: rx ry | word 0 of the last slot: the sum is the identity, word 1: the kind
template <class P, class F>
struct AffLab {
    static constexpr int C = F::LANES_PER_TASK;
    G16_HD static F ldf(const uint32_t* in, int slot, int hi) { return TableLane<F>::wrap(ld<P>(in, slot + hi)); }
    G16_HD static void run(const uint32_t* in, uint32_t* out, int hi) {
        const bool pz = in[0] != 0, qz = in[1] != 0;
        const F px = ldf(in, 1, hi), py = ldf(in, 1 + C, hi), qx = ldf(in, 1 + 2 * C, hi), qy = ldf(in, 1 + 3 * C, hi);
        F d, rx, ry;
        bool rz;
        const int kind = AffineBatch<F>::classify(pz, qz, px, py, qx, qy, d);
        const F inv_d = batch_inverse(d);
        AffineBatch<F>::finish(kind, px, py, qx, qy, inv_d, rx, ry, rz);
        st<P>(out, hi, TableLane<F>::comp(rx)); st<P>(out, C + hi, TableLane<F>::comp(ry));
        if (hi == 0) {
            uint32_t* fl = out + 2 * C * Fp30<P>::NL;
            G16_UNROLL for (int i = 0; i < Fp30<P>::NL; ++i) fl[i] = i == 0 ? (rz ? 1u : 0u) : i == 1 ? (uint32_t)kind : 0u;
        }
    }
};

// one tuple of a one-lane form
template <class P, int FORM>
struct LabOp {
    typedef Fp30<P> B;
    G16_HD static void run(const uint32_t* in, uint32_t* out) {
        auto L = [&](int k) { return ld<P>(in, k); };
        if constexpr (FORM == 0) st<P>(out, 0, L(0).mul(L(1)));
        else if constexpr (FORM == 1) st<P>(out, 0, L(0).sqr());
        else if constexpr (FORM == 2) st<P>(out, 0, B::mul_add_fused(L(0), L(1), L(2), L(3)));
        else if constexpr (FORM == 3) st<P>(out, 0, B::template mul4_cols<uint64_t>(L(0), L(1), L(2), L(3), L(4), L(5), L(6), L(7)));
        else if constexpr (FORM == 4) st<P>(out, 0, L(0).template mul_sub_k<2>(L(1), L(2)));
        else if constexpr (FORM == 5) st<P>(out, 0, B::template mul2_sub_k<2>(L(0), L(1), L(2), L(3), L(4)));
        else if constexpr (FORM == 6) st<P>(out, 0, L(0).template mul_sub_k<4>(L(1), L(2)));
        else if constexpr (FORM == 7) st<P>(out, 0, B::template mul2_sub_k<4>(L(0), L(1), L(2), L(3), L(4)));
        else if constexpr (FORM == 8) st<P>(out, 0, L(0).template mul_sub_k<8>(L(1), L(2)));
        else if constexpr (FORM == 9) st<P>(out, 0, B::template mul2_sub_k<8>(L(0), L(1), L(2), L(3), L(4)));
        else if constexpr (FORM == 10) st<P>(out, 0, L(0).mul_sub_x3(L(1), L(2), L(3)));
        else if constexpr (FORM == 11) st<P>(out, 0, L(0).sqr_sub_x3(L(1), L(2)));
        else if constexpr (FORM == 20) st<P>(out, 0, L(0).template sub<2>(L(1)));
        else if constexpr (FORM == 21) st<P>(out, 0, L(0).template sub<4>(L(1)));
        else if constexpr (FORM == 22) st<P>(out, 0, L(0).template sub<6>(L(1)));
        else if constexpr (FORM == 23) st<P>(out, 0, L(0).template sub<8>(L(1)));
        else if constexpr (FORM == 24) st<P>(out, 0, L(0).template sub<16>(L(1)));
        else if constexpr (FORM == 25) st<P>(out, 0, L(0).add_dbl(L(1)));
        else if constexpr (FORM == 26) { B a = L(0); a.normalize(); st<P>(out, 0, a); }
        else if constexpr (FORM == 27) {
            const int k = (int)in[2 * B::NL];
            st<P>(out, 0, L(0).sub_pow2(L(1), k < 0 ? 0 : k > 11 ? 11 : k));
        }
        else if constexpr (FORM == 28) {
            const Fp<P> y = ld_words<P>(in, 0);
            const bool flip = in[B::NL] != 0;
            st<P>(out, 0, B::unpack_cond_neg(y, flip));
            st<P>(out, 1, B::cond_neg2(B::unpack(y.v), flip));
        }
        else if constexpr (FORM == 30) st<P>(out, 0, L(0).template cond_sub<2>());
        else if constexpr (FORM == 31) st<P>(out, 0, L(0).template cond_sub<4>());
        else if constexpr (FORM == 32) st<P>(out, 0, L(0).template cond_sub<8>());
        else if constexpr (FORM == 33) st<P>(out, 0, L(0).template cond_sub<16>());
        else if constexpr (FORM == 34) st<P>(out, 0, L(0).weak_reduce32());
        else if constexpr (FORM == 35) st<P>(out, 0, L(0).canonical_lt2p());
        else if constexpr (FORM == 36) st<P>(out, 0, L(0).canonical_lt8p());
        else if constexpr (FORM == 37) st<P>(out, 0, L(0).canonical_quick());
        else if constexpr (FORM == 38) st<P>(out, 0, L(0).neg_canonical());
        else if constexpr (FORM == 39) st_flag<P>(out, 0, L(0).maybe_zero());
        else if constexpr (FORM == 40) st_flag<P>(out, 0, L(0).is_zero_exact());
        else if constexpr (FORM == 41) st_words<P>(out, 0, L(0).to_std());
        else if constexpr (FORM == 42) st_words<P>(out, 0, B::std_to_r30(ld_words<P>(in, 0)));
        else if constexpr (FORM == 43) st_words<P>(out, 0, L(0).to_packed());
        else if constexpr (FORM == 50) {
            const Fp2x30<P> a{L(0), L(1)}, b{L(2), L(3)};
            const Fp2x30<P> r = a.mul(b);
            st<P>(out, 0, r.c0); st<P>(out, 1, r.c1);
        }
        else if constexpr (FORM == 51) {
            const Fp2x30<P> a{L(0), L(1)};
            const Fp2x30<P> r = a.sqr();
            st<P>(out, 0, r.c0); st<P>(out, 1, r.c1);
        }
        else if constexpr (FORM == 70) AccLab<P, Fp30<P>>::run(in, out, 0);
        else if constexpr (FORM == 71) AccLab<P, Fp2x30<P>>::run(in, out, 0);
        else if constexpr (FORM == 73) {   // (the host twin: on the device devlab_op parks in LDS)
            AccParked<B, ParkedArrayStore<B>> a;
            ParkedLab<P, B, ParkedArrayStore<B>>::run(in, out, 0, a);
        }
        else if constexpr (FORM == 80) st<P>(out, 0, ModInv30<P>::inverse_plain(L(0)));
        else if constexpr (FORM == 81) st<P>(out, 0, batch_inverse(L(0)));
        else if constexpr (FORM == 83) JacLab<P, B>::run(in, out, 0);
        else if constexpr (FORM == 85) AffLab<P, B>::run(in, out, 0);
    }
};

// one lane's half of a lane-pair form: Fq2 operand k has its components in slots 2 k and 2 k + 1, the lane holds component `hi`
template <class P, int FORM>
struct LabPair {
    typedef Fp30<P> B;
    typedef Fp2p30<P> F;
#if defined(__HIP_DEVICE_COMPILE__)
    static __device__ __forceinline__ void run(const uint32_t* in, uint32_t* out) {
        const int hi = F::lane_hi() ? 1 : 0;
        if constexpr (FORM == 72) { AccLab<P, F>::run(in, out, hi); return; }
        if constexpr (FORM == 84) { JacLab<P, F>::run(in, out, hi); return; }
        if constexpr (FORM == 86) { AffLab<P, F>::run(in, out, hi); return; }
        auto L = [&](int k) { return F{ld<P>(in, 2 * k + hi)}; };
        F r = F::zero();
        if constexpr (FORM == 60) r = F::mul_v(F::lhs(L(0)), F::rhs(L(1)));
        else if constexpr (FORM == 61) r = F::sqr_v(F::lhs(L(0)));
        else if constexpr (FORM == 62) r = F::sqr_sub_x3_v(F::lhs(L(0)), L(1), L(2));
        else if constexpr (FORM == 63) r = F::mul_add_fused(L(0), L(1), L(2), L(3));
        else if constexpr (FORM == 64) r = F::mul_sub_fused(L(0), L(1), L(2), L(3));
        else if constexpr (FORM == 65) r = F::mul_add_fused_v(F::lhs(L(0)), F::rhs(L(1)), F::lhs(L(2)), F::rhs(L(3)));
        else if constexpr (FORM == 82) r = batch_inverse(L(0));
        st<P>(out, hi, r.c);
    }
#endif
    static void run_host(const uint32_t* in, uint32_t* out) {
        for (int h = 0; h < 2; ++h) {
            const bool hi = h != 0;
            auto C = [&](int k, int c) { return ld<P>(in, 2 * k + c); };
            auto y2 = [&](int k) { return hi ? C(k, 0) : C(k, 1).neg16(); };   // what the product takes from the partner lane
            B r = B::zero();
            if constexpr (FORM == 60) r = F::pair_mul_c(hi, C(0, 0), C(0, 1), C(1, h), C(1, 1 - h));
            else if constexpr (FORM == 61) r = F::pair_sqr_c(hi, C(0, 0), C(0, 1));
            else if constexpr (FORM == 62) r = F::pair_sqr_sub_x3(hi, C(0, 0), C(0, 1), C(1, h), C(2, h));
            else if constexpr (FORM == 63) r = F::pair_mul_add_c(hi, C(0, 0), C(0, 1), C(1, h), C(1, 1 - h), C(2, 0), C(2, 1), C(3, h), C(3, 1 - h));
            else if constexpr (FORM == 64) r = F::pair_mul_sub_c(hi, C(0, 0), C(0, 1), C(1, h), C(1, 1 - h), C(2, 0), C(2, 1), C(3, h), C(3, 1 - h));
            // (mul_add_fused_v has no pure per-lane routine: this line restates it, so on the host form 65 checks the restatement and
            //  the four-sweep product only; the device tier runs the project's own lhs / rhs / mul_add_fused_v)
            else if constexpr (FORM == 65) r = B::template mul4_cols<uint64_t>(C(0, 0), C(1, h), C(0, 1), y2(1), C(2, 0), C(3, h), C(2, 1), y2(3));
            else if constexpr (FORM == 82) r = pair_inverse<P>(hi, C(0, h), C(0, 1 - h));
            st<P>(out, h, r);
        }
    }
};

constexpr int LAB_WG = 64;   // one wavefront per workgroup: 65 tuples already span two workgroups

template <class P, int FORM>
__global__ void __launch_bounds__(LAB_WG) devlab_op(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    constexpr int NL = Fp30<P>::NL, NIN = lab_nin(FORM), NOUT = lab_nout(FORM);
    const uint32_t t = blockIdx.x * LAB_WG + threadIdx.x;
    if constexpr (lab_is_parked(FORM)) {
#if defined(__HIP_DEVICE_COMPILE__)
        // the bucket pass's LDS layout: 4 * NL * 64 words per 64-lane workgroup, every lane its own column (no barrier needed)
        typedef typename std::conditional<lab_is_pair(FORM), Fp2p30<P>, Fp30<P>>::type F;
        static_assert(LAB_WG == ACC_THREADS, "LdsAccStore is laid out for ACC_THREADS lanes");
        __shared__ __attribute__((aligned(16))) uint32_t acc_lds[4 * F::PREFIX_LIMBS * ACC_THREADS];
        constexpr uint32_t LPT = F::LANES_PER_TASK;
        if (t >= LPT * n) return;   // both lanes of a pair leave together
        const size_t i = t / LPT;
        AccParked<F, LdsAccStore<F>> acc;
        acc.s.quad = acc_lds + 4 * threadIdx.x;
        acc.s.tail = acc_lds + 4 * LdsAccStore<F>::QUADS * ACC_THREADS + threadIdx.x;
        ParkedLab<P, F, LdsAccStore<F>>::run(in + i * NIN * NL, out + i * NOUT * NL, LPT == 2 && (threadIdx.x & 1u) ? 1 : 0, acc);
#endif
    } else if constexpr (lab_is_pair(FORM)) {
        if (t >= 2 * n) return;   // both lanes of a pair leave together
        const size_t i = t >> 1;
#if defined(__HIP_DEVICE_COMPILE__)
        LabPair<P, FORM>::run(in + i * NIN * NL, out + i * NOUT * NL);
#endif
    } else {
        if (t >= n) return;
        LabOp<P, FORM>::run(in + (size_t)t * NIN * NL, out + (size_t)t * NOUT * NL);
    }
}

template <class P, int FORM>
int lab_device(hipStream_t st, const uint32_t* operands, uint64_t n, uint32_t* out) {
    constexpr int NL = Fp30<P>::NL, NIN = lab_nin(FORM), NOUT = lab_nout(FORM);
    const size_t in_bytes = (size_t)n * NIN * NL * 4, out_bytes = (size_t)n * NOUT * NL * 4;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    G16_HIP_TRY(hipMalloc((void**)&d_in, in_bytes));
    if (hipMalloc((void**)&d_out, out_bytes) != hipSuccess) { (void)hipFree(d_in); return G16_ERR_OOM; }
    auto body = [&]() -> int {
        G16_HIP_TRY(hipMemcpyAsync(d_in, operands, in_bytes, hipMemcpyHostToDevice, st));
        G16_HIP_TRY(hipMemsetAsync(d_out, 0, out_bytes, st));
        const uint64_t lanes = lab_is_pair(FORM) ? 2 * n : n;
        devlab_op<P, FORM><<<dim3((unsigned)((lanes + LAB_WG - 1) / LAB_WG)), dim3(LAB_WG), 0, st>>>(d_in, d_out, (uint32_t)n);
        G16_LAUNCH_CHECK();
        G16_HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
        G16_HIP_TRY(hipStreamSynchronize(st));
        return G16_OK;
    };
    const int rc = body();
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

template <class P, int FORM>
int lab_host(const uint32_t* operands, uint64_t n, uint32_t* out) {
    constexpr int NL = Fp30<P>::NL, NIN = lab_nin(FORM), NOUT = lab_nout(FORM);
    for (uint64_t i = 0; i < n; ++i) {
        if constexpr (lab_is_pair(FORM)) LabPair<P, FORM>::run_host(operands + i * NIN * NL, out + i * NOUT * NL);
        else LabOp<P, FORM>::run(operands + i * NIN * NL, out + i * NOUT * NL);
    }
    return G16_OK;
}

#define LAB_FORMS(X)                                                                                                              \
    X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(30) X(31) \
    X(32) X(33) X(34) X(35) X(36) X(37) X(38) X(39) X(40) X(41) X(42) X(43) X(50) X(51) X(60) X(61) X(62) X(63) X(64) X(65) X(70) X(71) X(72) X(73) X(74) \
    X(80) X(81) X(82) X(83) X(84) X(85) X(86)

// device: launch on st; otherwise the host twin (which has no lanes: the lane pair's accumulators, doublings and affine pairs, forms
// 72, 74, 84 and 86, are device forms)
template <class P>
int lab_dispatch(bool device, hipStream_t st, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    switch (form) {
#define X(F)                                                                                   \
    case F:                                                                                    \
        if constexpr (lab_has<P>(F)) {                                                         \
            if (device) return lab_device<P, F>(st, operands, n, out);                         \
            if constexpr (lab_device_only(F)) return G16_ERR_BAD_ARG;                                  \
            else return lab_host<P, F>(operands, n, out);                                      \
        } else return G16_ERR_BAD_ARG;
        LAB_FORMS(X)
#undef X
        default: return G16_ERR_BAD_ARG;
    }
}

int lab_run(int curve, bool device, hipStream_t st, int field, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    int nin = 0, nout = 0;
    if (!operands || !out || n == 0 || n > ((uint64_t)1 << 22) || (field != 0 && field != 1) || !lab_slots(form, &nin, &nout)) return G16_ERR_BAD_ARG;
    if (curve == G16_BLS12_381)
        return field ? lab_dispatch<Bls12_381FqP>(device, st, form, operands, n, out) : lab_dispatch<Bls12_381FrP>(device, st, form, operands, n, out);
    if (curve == G16_BN254)
        return field ? lab_dispatch<Bn254FqP>(device, st, form, operands, n, out) : lab_dispatch<Bn254FrP>(device, st, form, operands, n, out);
    return G16_ERR_BAD_ARG;
}

}  // namespace

extern "C" int g16_dev_fp30_op(g16_ctx* ctx, int field, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    int curve = 0;
    std::vector<int> devs;
    std::vector<hipStream_t> streams;
    G16_TRY(ctx_devices(ctx, &curve, devs, streams));
    G16_HIP_TRY(hipSetDevice(devs[0]));
    return lab_run(curve, true, streams[0], field, form, operands, n, out);
}

extern "C" int g16_host_fp30_op(int curve, int field, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    return lab_run(curve, false, nullptr, field, form, operands, n, out);
}
