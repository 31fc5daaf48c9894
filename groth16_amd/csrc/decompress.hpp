// Compressed curve points -> affine points, host + device, on the fields of pairing.hpp.
//
// What Proof::deserialize_compressed does per point before any validation (src/data_structures.rs:8-16 derives
// CanonicalDeserialize for A | B | C), by exactly the rules of PointIo::read(compressed = true, validate = 0) in serialize.hip:
//   BLS12-381   zcash form: big-endian, Fq2 as c1 | c0, flags in the FIRST byte: 0x80 compressed (must be set), 0x40 infinity, 0x20 y is the
//               larger of {y, -y}
//   BN254       ark-serialize form: little-endian, Fq2 as c0 | c1, flags in the LAST byte: 0x80 y is the larger, 0x40 infinity
// In both forms the flags sit in the most significant byte of x (of x.c1 for Fq2).  Status 0 (the path's G16_ERR_INVALID_DATA): a
// coordinate >= p, BLS12-381 without the compressed bit, infinity with x != 0, infinity together with the sign flag, an x for
// which x^3 + b has no square root.  Status 1: the affine point in the ABI's Montgomery limbs, the identity all-zero; y is the one
// of +-y with is_larger_than_neg(y) == flag ("larger" on canonical integers, Fq2 by c1 first, then c0), so the result does not
// depend on which root the algorithm meets.  A point of status 0 is written as the identity.
//
// Square roots.  Both base fields have p = 3 (mod 4).  ONE exponentiation serves everything: t = a^((p - 3) / 4), out of line, a
// public exponent (every lane walks the same bits).  With r = t a:  r^2 = a * a^((p - 1) / 2) = +-a  and  t r = a^((p - 1) / 2) = +-1.
//   Fq    r is the root iff r^2 == a.
//   Fq2   the norm method of FieldIo<Fp2>::sqrt without its two Fermat inversions and without its second candidate:
//         s = sqrt(a0^2 + a1^2) in Fq (none: a is no square), d = (a0 + s) / 2, t = d^((p - 3) / 4), r = t d.
//           r^2 ==  d:  d is a square, 1 / r =  t, root = (r, a1 t / 2)                     [x0 = r, x1 = a1 / (2 x0)]
//           r^2 == -d:  d is none, so d' = (a0 - s) / 2 = -a1^2 / (4 d) is (-1 is none); 1 / r = -t and
//                       sqrt(d') = a1 / (2 r) = -a1 t / 2,  x1 = a1 / (2 x0) = r:  root = (-a1 t / 2, r)
//         a1 == 0: r = t a0 gives r^2 = +-a0: root (r, 0) or (0, r).  Two exponentiations per G2 point, one per G1 point, where
//         the one-exponentiation "complex" method spends two Fq2 exponentiations (about 2.3 times the Fq products).  The candidate
//         is checked by squaring, so a wrong branch can only answer "no root".
#pragma once
#include "../../include/g16_mi355x.h"
#include "pairing.hpp"

namespace g16 {

template <class C>
struct Decompress {
    typedef Pairing<C> PP;
    typedef typename PP::K K;
    typedef typename PP::P P;
    typedef typename PP::F F;
    typedef typename PP::F2 F2;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    static constexpr bool ZCASH = C::CURVE_ID == G16_BLS12_381;   // big-endian, flags in the first byte
    static constexpr int FQ_BYTES = (P::BITS + 7) / 8;
    static constexpr int G1_BYTES = FQ_BYTES, G2_BYTES = 2 * FQ_BYTES;
    static constexpr uint8_t FLAG_BITS = ZCASH ? 0xe0 : 0xc0;
    static_assert((P::mod(0) & 3u) == 3u, "the square roots below need p = 3 (mod 4)");

    struct Flags { bool ok, inf, larger; };
    // top: the most significant byte of x (x.c1)
    G16_HD static Flags flags(uint8_t top) {
        if constexpr (ZCASH) return {(top & 0x80) != 0 && !((top & 0x40) && (top & 0x20)), (top & 0x40) != 0, (top & 0x20) != 0};
        else return {!((top & 0x40) && (top & 0x80)), (top & 0x40) != 0, (top & 0x80) != 0};
    }
    // one coordinate (flag bits cleared when it carries them); false if the integer is >= p
    G16_HD static bool read_fq(const uint8_t* in, bool flagged, Fq* out) {
        uint32_t w[Fq::N];
        G16_UNROLL for (int i = 0; i < Fq::N; ++i) w[i] = 0;
        G16_UNROLL for (int i = 0; i < FQ_BYTES; ++i) {
            uint8_t b = in[ZCASH ? FQ_BYTES - 1 - i : i];
            if (i == FQ_BYTES - 1 && flagged) b &= (uint8_t)~FLAG_BITS;
            w[i >> 2] |= (uint32_t)b << (8 * (i & 3));
        }
        bool below = false, decided = false;
        G16_UNROLL for (int i = Fq::N - 1; i >= 0; --i)
            if (!decided && w[i] != P::mod(i)) { below = w[i] < P::mod(i); decided = true; }
        if (!below) return false;
        *out = Fq::from_canonical(w);
        return true;
    }
    // -1, 0, 1 comparing canonical integers
    G16_HD static int cmp(const Fq& a, const Fq& b) {
        uint32_t x[Fq::N], y[Fq::N];
        a.to_canonical(x);
        b.to_canonical(y);
        int r = 0;
        G16_UNROLL for (int i = 0; i < Fq::N; ++i)
            if (x[i] != y[i]) r = x[i] < y[i] ? -1 : 1;
        return r;
    }
    G16_HD static bool is_larger_than_neg(const Fq& y) { return cmp(y, y.neg()) > 0; }
    G16_HD static bool is_larger_than_neg(const Fq2& y) {
        const int c = cmp(y.c1, y.c1.neg());
        return c ? c > 0 : cmp(y.c0, y.c0.neg()) > 0;
    }

    // a^((p - 3) / 4): bit k of the exponent is bit k + 2 of p
    G16_HD_NOINLINE static F pow_pm3_4(const F& a) {
        F r = F::one();
#pragma nounroll
        for (int k = P::BITS - 3; k >= 0; --k) {
            r = r.sqr();
            if ((P::mod((k + 2) >> 5) >> ((k + 2) & 31)) & 1u) r = r * a;
        }
        return r;
    }
    G16_HD static bool sqrt(const F& a, F& out) {
        out = pow_pm3_4(a) * a;
        return out.sqr() == a;
    }
    G16_HD static bool sqrt(const F2& a, F2& out) {
        if (a.c1.is_zero()) {
            const F r = pow_pm3_4(a.c0) * a.c0;
            const F sq = r.sqr();
            if (sq == a.c0) { out = {r, F::zero()}; return true; }
            if ((sq + a.c0).is_zero()) { out = {F::zero(), r}; return true; }
            return false;
        }
        F s;
        if (!sqrt(a.c0.sqr() + a.c1.sqr(), s)) return false;
        const F d = (a.c0 + s) * PP::two_inv();
        const F t = pow_pm3_4(d);
        const F r = t * d, h = a.c1 * t * PP::two_inv();
        if (r.sqr() == d) out = {r, h};
        else out = {h.neg(), r};
        return out.sqr() == a;
    }

    G16_HD static uint8_t g1(const uint8_t* in, typename C::G1A* out) {
        *out = C::G1A::identity();
        const Flags fl = flags(in[ZCASH ? 0 : G1_BYTES - 1]);
        Fq x;
        if (!fl.ok || !read_fq(in, true, &x)) return 0;
        if (fl.inf) return x.is_zero() ? 1 : 0;
        const F xm = F::from_std(x);
        F y;
        if (!sqrt(xm.sqr() * xm + F::from_std(C::b1()), y)) return 0;
        Fq ys = y.to_std();
        if (is_larger_than_neg(ys) != fl.larger) ys = ys.neg();
        *out = {x, ys};
        return 1;
    }
    G16_HD static uint8_t g2(const uint8_t* in, typename C::G2A* out) {
        *out = C::G2A::identity();
        const Flags fl = flags(in[ZCASH ? 0 : G2_BYTES - 1]);
        Fq2 x;
        if (!fl.ok) return 0;
        if (!read_fq(in, ZCASH, ZCASH ? &x.c1 : &x.c0) || !read_fq(in + FQ_BYTES, !ZCASH, ZCASH ? &x.c0 : &x.c1)) return 0;
        if (fl.inf) return x.is_zero() ? 1 : 0;
        const F2 xm = PP::f2_std(x);
        F2 y;
        if (!sqrt(xm.sqr() * xm + PP::twist_b(), y)) return 0;
        Fq2 ys = {y.c0.to_std(), y.c1.to_std()};
        if (is_larger_than_neg(ys) != fl.larger) ys = ys.neg();
        *out = {x, ys};
        return 1;
    }

    // ---- the uncompressed forms: x | y, by the rules of PointIo::read(compressed = false, ...) in serialize.hip -------------------
    //   BLS12-381   flags in the first byte of x (x.c1): 0x80 must be clear, 0x20 (a sign has no place here) must be clear, 0x40 infinity
    //   BN254       flags in the last byte of y (y.c1): 0x40 infinity, 0x80 the sign of y -- refused together with infinity, and NOT held
    //               against y on a finite point (the host reader does not look at it either)
    // Status 0: those flag rules, a coordinate >= p, infinity with x != 0 or y != 0.  Status 2 (only when check_curve is set, the
    // reader's validate >= 1): a finite point that does not satisfy the curve equation; x = y = 0 without the infinity flag is such a
    // point, although it has the identity's limbs.  Without check_curve whatever decodes is status 1, as on the host.
    struct RawFlags { bool ok, inf; };
    // top: the byte that carries the flags
    G16_HD static RawFlags raw_flags(uint8_t top) {
        if constexpr (ZCASH) return {(top & 0x80) == 0 && (top & 0x20) == 0, (top & 0x40) != 0};
        else return {!((top & 0x40) && (top & 0x80)), (top & 0x40) != 0};
    }
    G16_HD static uint8_t g1_raw(const uint8_t* in, bool check_curve, typename C::G1A* out) {
        *out = C::G1A::identity();
        const RawFlags fl = raw_flags(in[ZCASH ? 0 : 2 * G1_BYTES - 1]);
        typename C::G1A p;
        if (!fl.ok || !read_fq(in, ZCASH, &p.x) || !read_fq(in + FQ_BYTES, !ZCASH, &p.y)) return 0;
        if (fl.inf) return p.is_identity() ? 1 : 0;
        if (check_curve && (p.is_identity() || !PP::g1_on_curve(p))) return 2;
        *out = p;
        return 1;
    }
    // (out may be the point's place in device memory, 16-byte aligned: the four coordinates are stored BEFORE the curve equation is
    // evaluated and taken back if it fails, so that they need not stay in registers beside its Fq2 products)
    G16_HD static uint8_t g2_raw(const uint8_t* in, bool check_curve, typename C::G2A* out) {
        *out = C::G2A::identity();
        const RawFlags fl = raw_flags(in[ZCASH ? 0 : 2 * G2_BYTES - 1]);
        typename C::G2A p;
        if (!fl.ok) return 0;
        if (!read_fq(in, ZCASH, ZCASH ? &p.x.c1 : &p.x.c0) || !read_fq(in + FQ_BYTES, false, ZCASH ? &p.x.c0 : &p.x.c1)) return 0;
        if (!read_fq(in + 2 * FQ_BYTES, false, ZCASH ? &p.y.c1 : &p.y.c0) || !read_fq(in + 3 * FQ_BYTES, !ZCASH, ZCASH ? &p.y.c0 : &p.y.c1))
            return 0;
        if (fl.inf) return p.is_identity() ? 1 : 0;
        *out = p;
        if (check_curve && (p.is_identity() || !PP::g2_on_curve(p))) {
            *out = C::G2A::identity();
            return 2;
        }
        return 1;
    }
};

// What a point's status byte becomes once its membership flag (subgroup.hpp: 1 member, 0 on the curve but outside the subgroup, 2 off
// the curve) is known -- the status codes of g16_decode_points: 1 passed, 0 the bytes do not decode, 2 off the curve, 3 outside the
// subgroup.  A point that did not decode keeps its status (it was stored as the identity, which every membership test passes).
G16_HD uint8_t decode_status_with_flag(uint8_t status, uint8_t flag) {
    if (status != 1 || flag == 1) return status;
    return flag == 2 ? 2 : 3;
}

// a proof decodes iff its three points do
G16_HD uint8_t decompress_proof_status(uint8_t a, uint8_t b, uint8_t c) { return (a == 1 && b == 1 && c == 1) ? 1 : 0; }

}  // namespace g16
