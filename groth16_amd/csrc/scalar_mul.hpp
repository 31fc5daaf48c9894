// out = k * P for one point and one scalar per task (libg16_phase1.so): the arithmetic of one task, written once for
// the device (one lane per G1 point, a lane pair per G2 point) and for the host emulation that the CPU tests run.
//
//   * a fixed signed 4-bit window: k + 0x88..8 is formed once, nibble j of it minus 8 is the digit d_j in [-8, 7], k = sum d_j 16^j
//     over 64 digits (r + 0x88..8 < 2^256 for both curves: no 65th digit).  Every task runs 252 doublings and 64 additions whatever
//     its scalar: a digit only chooses which table entry is read and its sign;
//   * ONE coordinate system, XYZZ in the 30-bit lazy arithmetic with the formulas and constants of Acc30 (fp30.hpp), whose bounds
//     the host self-test derives -- the table entries are XYZZ too, so an addition is add-2008-s (12 products + 2 squarings);
//   * the table 1P .. 8P (4 doublings, 3 additions) is parked limb-planar in HBM (IO::put / get: every load and store of a wave
//     touches consecutive words), and an entry's coordinates are fetched where a product consumes them;
//   * digit 0, an identity accumulator, an identity entry and an identity input are SELECTIONS between the old value, the entry and
//     the formula's result -- no lane branches on its own data.  The formulas run on whatever such a lane holds; what they
//     give there is never selected;
//   * an addition whose operands are equal or opposite (P = +-Q: possible only for points outside the prime-order subgroup, whose
//     small multiples repeat) is found by the exact zero test of U2 - U1; a vote decides per wave whether anyone needs the slow
//     path, which is the SAME doubling code run once more for the lanes that asked (one copy of each formula in the kernel);
//   * one field inversion per point (Bernstein-Yang, batch_affine.hpp) of zz * zzz.
// Products per scalar multiplication (squarings counted as products): table 4 * 9 + 3 * 14 = 78, loop 252 * 9 + 64 * 14 = 3164,
// exit 5 + 2 conversions: 3249, plus one inversion.
#pragma once
#include "fp30.hpp"
#include "batch_affine.hpp"
#include "window_tables.hpp"

namespace g16 {

constexpr int SMUL_ENTRIES = 8;                  // 1P .. 8P
constexpr int SMUL_DIGITS = 64;                  // signed 4-bit digits of a 256-bit scalar
constexpr int SMUL_SLOTS = 4 * SMUL_ENTRIES;     // parked field elements per task lane
constexpr int SMUL_KWORDS = 8;                   // words of the biased scalar, parked behind the table
constexpr uint32_t SMUL_BIAS = 0x88888888u;

// k (canonical, 8 words) + 0x88..8; false if the sum does not fit 256 bits (never for k < r of the supported curves)
G16_HD bool smul_bias(const uint32_t k[SMUL_KWORDS], uint32_t kb[SMUL_KWORDS]) {
    uint64_t c = 0;
    G16_UNROLL for (int i = 0; i < SMUL_KWORDS; ++i) {
        c += (uint64_t)k[i] + SMUL_BIAS;
        kb[i] = (uint32_t)c;
        c >>= 32;
    }
    return c == 0;
}

template <class F>
struct SmulAcc {
    F x, y, zz, zzz;   // between calls: x < 7.5p, y <= 4p (a negated entry taken as it is), zz, zzz < 1.8p per component
    bool inf;
};

// a <- 2 a where `on`, else unchanged.  dbl-2008-s-1 as Acc30::dbl; y = 0 (a point of order two) gives the identity.
template <class F, class IO>
G16_HD void smul_dbl(IO& io, SmulAcc<F>& a, bool on) {
    const F U = a.y.dbl();                                   // <= 8p
    const bool z = io.is_zero(U);
    const F V = U.sqr();
    const F W = U.mul(V);
    const F S = a.x.mul(V);
    const F X2 = a.x.sqr();
    const F M = X2.dbl().add(X2);
    const F X3 = M.sqr().template sub<F::K2M>(S.dbl());
    const F Y3 = F::mul_sub(M, S.template sub<F::KX>(X3), a.y, W);
    a.x = io.select(on, X3, a.x);
    a.y = io.select(on, Y3, a.y);
    a.zz = io.select(on, V.mul(a.zz), a.zz);
    a.zzz = io.select(on, W.mul(a.zzz), a.zzz);
    a.inf = a.inf || (on && z);
}

// the entry's y, negated for a negative digit: 4p - y for y < 3.5p (an affine input: < p)
template <class F, class IO>
G16_HD F smul_entry_y(IO& io, int e, bool minus) {
    const F y = io.get(e + 1);
    return io.select(minus, F::zero().template sub<4>(y), y);
}

// a <- a + (+-entry at slots e .. e + 3), add-2008-s as Acc30::add / acc_add_streamed.  e_none: the entry is the identity or the
// digit is zero.  Returns the lanes whose two operands are the SAME point: their accumulator is untouched and the caller doubles it.
template <class F, class IO>
G16_HD bool smul_add(IO& io, SmulAcc<F>& a, int e, bool e_none, bool minus) {
    const bool take = a.inf && !e_none;      // identity + entry
    const bool live = !a.inf && !e_none;
    const F U1 = a.x.mul(io.get(e + 2));
    const F S1 = a.y.mul(io.get(e + 3));
    const F Pd = io.get(e + 0).template mul_sub_k<F::KM>(a.zz, U1);                  // U2 - U1
    const F R = smul_entry_y<F>(io, e, minus).template mul_sub_k<F::KM>(a.zzz, S1);  // S2 - S1
    const bool same_x = io.is_zero(Pd) && live;
    bool same = false;
    if (io.any(same_x)) {   // decided per wave; equal or opposite operands need a point outside the prime-order subgroup
        const bool rz = io.is_zero(R);
        same = same_x && rz;
        a.inf = a.inf || (same_x && !rz);    // opposite: the sum is the identity
    }
    const bool keep = e_none || same_x;
    const F PP = Pd.sqr();
    const F PPP = Pd.mul(PP);
    {
        const F ezz = io.get(e + 2);
        a.zz = io.select(keep, a.zz, io.select(take, ezz, a.zz.mul(ezz).mul(PP)));
    }
    {
        const F ezzz = io.get(e + 3);
        a.zzz = io.select(keep, a.zzz, io.select(take, ezzz, a.zzz.mul(ezzz).mul(PPP)));
    }
    const F Q = U1.mul(PP);
    static_assert(F::KM + F::K2M == 6, "sqr_sub_x3 subtracts from 6 p");
    const F X3 = R.sqr_sub_x3(PPP, Q);
    const F Y3 = F::mul_sub(R, Q.template sub<F::KX>(X3), S1, PPP);
    a.x = io.select(keep, a.x, io.select(take, io.get(e + 0), X3));
    a.y = io.select(keep, a.y, io.select(take, smul_entry_y<F>(io, e, minus), Y3));
    a.inf = keep && a.inf;
    return same;
}

// IO: where the task's data lives and how its lanes agree
//   bool load(F& x, F& y)          the point in the R' radix, canonical; false for the identity
//   uint32_t kword(int w)          word w of the biased scalar (smul_bias)
//   void put(int slot, v) / F get(int slot)      SMUL_SLOTS parking slots
//   bool is_zero(v)                exact test of a lazy value (< 16p per component), the same in every lane of the task
//   bool any(bool)                 true if any task that shares the wave says so
//   F select(bool c, a, b)         c ? a : b without a branch
//   void store(x, y, identity)     lazy coordinates (< 16p) out, converted to the caller's form
template <class F, class IO>
G16_HD void scalar_mul_task(IO& io) {
    SmulAcc<F> a;
    uint32_t none;   // bit m: entry m P is the identity (bit 0: digit zero adds nothing)
    {
        F px, py;
        const bool finite = io.load(px, py);
        none = finite ? 1u : 0x1ffu;
        io.put(0, px); io.put(1, py); io.put(2, F::one()); io.put(3, F::one());
        a.x = px; a.y = py; a.zz = F::one(); a.zzz = F::one(); a.inf = !finite;
    }
    // steps 0 .. 6 build entry m = step + 2 (even: the double of m / 2, odd: entry m - 1 plus P); steps 7 .. 70 are the digits from
    // the top: add the digit's entry, then four doublings (none after the last)
    for (int step = 0; step < SMUL_ENTRIES - 1 + SMUL_DIGITS; ++step) {
        const bool table = step < SMUL_ENTRIES - 1;
        const int m = step + 2;
        int e, ndbl;
        bool add, e_none, minus;
        if (table) {
            const int src = (m & 1) ? m - 1 : m >> 1;
            a.x = io.get(4 * (src - 1) + 0); a.y = io.get(4 * (src - 1) + 1); a.zz = io.get(4 * (src - 1) + 2); a.zzz = io.get(4 * (src - 1) + 3);
            a.inf = (none >> src) & 1u;
            add = (m & 1) != 0;
            e = 0; e_none = (none >> 1) & 1u; minus = false;
            ndbl = add ? 0 : 1;
        } else {
            const int j = SMUL_ENTRIES - 1 + SMUL_DIGITS - 1 - step;   // 63 .. 0
            if (j == SMUL_DIGITS - 1) a.inf = true;
            const int d = (int)((io.kword(j >> 3) >> (4 * (j & 7))) & 15u) - 8;
            const int mag = d < 0 ? -d : d;
            add = true;
            minus = d < 0;
            e = mag ? 4 * (mag - 1) : 0;
            e_none = (none >> mag) & 1u;
            ndbl = j ? 4 : 0;
        }
        bool again = false;
        if (add) again = smul_add<F>(io, a, e, e_none, minus);
        for (int k = -1; k < ndbl; ++k) {
            if (k < 0 && !io.any(again)) continue;    // nobody in the wave added a point to itself
            smul_dbl<F>(io, a, k >= 0 || again);
        }
        if (table) {
            io.put(4 * (m - 1) + 0, a.x); io.put(4 * (m - 1) + 1, a.y); io.put(4 * (m - 1) + 2, a.zz); io.put(4 * (m - 1) + 3, a.zzz);
            none |= (a.inf ? 1u : 0u) << m;
        }
    }
    // x / zz, y / zzz from ONE inversion: i = 1 / (zz zzz), 1 / zz = i zzz, 1 / zzz = i zz  (an identity's inverse of zero is zero)
    const F inv = batch_inverse(a.zz.mul(a.zzz));
    const F ax = a.x.mul(inv.mul(a.zzz));
    const F ay = a.y.mul(inv.mul(a.zz));
    io.store(ax, ay, a.inf);
}

// ---- device side ------------------------------------------------------------------------------------------------------------
// src / dst: packed base-field elements of one point (x parts, then y parts), standard Montgomery form; park: slot s, limb l of this
// lane at park[(s * NL + l) * stride], word w of the biased scalar at kpark[w * stride]
template <class F30>
struct SmulDeviceIO {
    typedef TableLane<F30> TL;
    typedef typename TL::B B;
    typedef typename B::Std W32;
    static constexpr int NL = B::NL;
    const W32* src;
    W32* dst;
    uint32_t* park;
    const uint32_t* kpark;
    uint64_t stride;
    G16_HD bool load(F30& x, F30& y) const {
        const int k = TL::part();
        const W32 xs = src[k], ys = src[TL::PARTS + k];
        const bool finite = !TL::all(xs.is_zero() && ys.is_zero());
        // x R -> x R' as B::std_to_r30, with the standard product INLINED: the out-of-line one of the wide field is the only call
        // of the kernel and would give it a stack (160 bytes of scratch per lane)
        W32 c;
        G16_UNROLL for (int i = 0; i < W32::N; ++i) c.v[i] = B::Params_t::r30_plain(i);
        x = TL::wrap(B::unpack(xs.mul_inlined(c).v));
        y = TL::wrap(B::unpack(ys.mul_inlined(c).v));
        return finite;
    }
    G16_HD uint32_t kword(int w) const { return kpark[(uint64_t)w * stride]; }
    G16_HD void put(int slot, const F30& v) const {
        const B& b = TL::comp(v);
        G16_UNROLL for (int l = 0; l < NL; ++l) park[((uint64_t)slot * NL + l) * stride] = b.l[l];
    }
    G16_HD F30 get(int slot) const {
        B b;
        G16_UNROLL for (int l = 0; l < NL; ++l) b.l[l] = park[((uint64_t)slot * NL + l) * stride];
        return TL::wrap(b);
    }
    G16_HD bool any(bool v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return __ballot(v) != 0;
#else
        return v;
#endif
    }
    // the cheap filter in every lane, the exact comparison only where some lane of the wave passed it
    G16_HD bool is_zero(const F30& v) const {
        bool z = TL::all(TL::comp(v).maybe_zero());
        if (any(z)) {
            const bool exact = TL::all(TL::comp(v).is_zero_exact());
            z = z && exact;
        }
        return z;
    }
    G16_HD F30 select(bool c, const F30& a, const F30& b) const {
        B r;
        G16_UNROLL for (int l = 0; l < NL; ++l) r.l[l] = c ? TL::comp(a).l[l] : TL::comp(b).l[l];
        return TL::wrap(r);
    }
    G16_HD void store(const F30& x, const F30& y, bool identity) const {
        const int k = TL::part();
        const W32 xs = TL::comp(x).to_std(), ys = TL::comp(y).to_std();
        dst[k] = identity ? W32::zero() : xs;
        dst[TL::PARTS + k] = identity ? W32::zero() : ys;
    }
};

}  // namespace g16
