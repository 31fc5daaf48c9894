// Prime-order subgroup membership of affine curve points, host + device, on the fields of pairing.hpp.
//
// The point checks of Validate::Yes (ark-serialize's is_in_correct_subgroup_assuming_on_curve) without a multiplication by r:
// each test compares an efficiently computable endomorphism of the point with a short PUBLIC multiple of it, so every lane of a
// wave runs the same double-and-add instruction stream (no per-lane bit tests).
//
//   BLS12-381 G1   phi(P) = -[x^2] P     phi(x, y) = (beta x, y); two chains over |x| (Scott, eprint 2021/1130; valid for this
//                                        curve by eprint 2022/352)
//   BLS12-381 G2   psi(Q) = [x] Q        psi = twist o Frobenius o untwist on the M-type twist; x < 0, so compared with -[|x|] Q
//   BN254 G1       cofactor 1            every curve point is a member
//   BN254 G2       psi(Q) = [6x^2] Q     psi = Pairing::frob_twist(Q, 1); a 127-bit chain (eprint 2022/352, section 4.3)
//
// beta, psi's coefficients and 6x^2 come from gen_params.py, which checks each identity on the generator with big integers.
// The input may be ANY point of the curve: a point of order 3 gives [2]P = -P and the next addition the identity, points of
// order 11 or 13 meet P + P and P - P inside a 64-step chain.  XYZZ's dbl / add / add_affine are complete (they test for the
// identity, for equal and for opposite operands), so the chains are exact on such inputs.  The comparison is projective
// (cross-multiplied): no field inverse per point.
#pragma once
#include "pairing.hpp"

namespace g16 {

template <class C>
struct Subgroup {
    typedef Pairing<C> PP;
    typedef typename PP::K K;
    typedef typename PP::F F;
    typedef typename PP::F2 F2;
    typedef typename PP::A1 A1;
    typedef typename PP::A2 A2;

    template <class E>
    G16_HD static void acc_add(XYZZ<E>& acc, const Affine<E>& p) { acc.add_affine(p); }
    template <class E>
    G16_HD static void acc_add(XYZZ<E>& acc, const XYZZ<E>& p) { acc.add(p); }

    // [k] p for the public k = hi 2^64 + lo > 0 (the same for every lane: the bit tests are uniform branches)
    template <class E, class Base>
    G16_HD static XYZZ<E> mul_public(const Base& p, uint64_t hi, uint64_t lo) {
        int top = 127;
        while (!(((top >= 64 ? hi >> (top - 64) : lo >> top)) & 1u)) --top;
        XYZZ<E> acc = XYZZ<E>::identity();
        acc_add(acc, p);
#pragma nounroll
        for (int i = top - 1; i >= 0; --i) {
            acc = acc.dbl();
            if (((i >= 64 ? hi >> (i - 64) : lo >> i)) & 1u) acc_add(acc, p);
        }
        return acc;
    }

    // (ex, ey) == +-(r.x / r.zz, r.y / r.zzz), cross-multiplied; the identity equals no affine point
    template <class E>
    G16_HD static bool same_point(const E& ex, const E& ey, const XYZZ<E>& r, bool negated) {
        if (r.is_identity()) return false;
        if (ex * r.zz != r.x) return false;
        const E s = ey * r.zzz;
        return negated ? (s + r.y).is_zero() : s == r.y;
    }

    // p: on the curve, not the identity
    G16_HD static bool g1_member(const A1& p) {
        if constexpr (PP::M_TWIST) {
            const XYZZ<F> t = mul_public<F>(Affine<F>{p.x, p.y}, 0, K::ATE_X_ABS);
            const XYZZ<F> r = mul_public<F>(t, 0, K::ATE_X_ABS);   // [x^2] p; the identity for p of order dividing x^2
            const F beta = F::konst([](int i) { return K::endo_beta30(0, i); });
            return same_point(beta * p.x, p.y, r, true);
        } else {
            return true;   // BN254: #E(Fq) = r, the cofactor is 1 -- on-curve is membership, no arithmetic
        }
    }
    G16_HD static bool g2_member(const A2& q) {
        if constexpr (PP::M_TWIST) {
            const F2 cx = {F::konst([](int i) { return K::psi30(0, i); }), F::konst([](int i) { return K::psi30(1, i); })};
            const F2 cy = {F::konst([](int i) { return K::psi30(2, i); }), F::konst([](int i) { return K::psi30(3, i); })};
            const XYZZ<F2> r = mul_public<F2>(Affine<F2>{q.x, q.y}, 0, K::ATE_X_ABS);
            static_assert(!PP::M_TWIST || K::ATE_X_NEG, "psi(Q) = [x] Q is compared with -[|x|] Q");
            return same_point(q.x.conj() * cx, q.y.conj() * cy, r, true);
        } else {
            const XYZZ<F2> r = mul_public<F2>(Affine<F2>{q.x, q.y}, K::G2_ENDO_HI, K::G2_ENDO_LO);
            const A2 e = PP::frob_twist(q, 1);
            return same_point(e.x, e.y, r, false);
        }
    }

    // the flag byte of the ABI: 1 in the subgroup (the identity included), 0 on the curve but outside it, 2 off the curve
    G16_HD static uint8_t g1_flag(const typename C::G1A& p) {
        if (!PP::g1_on_curve(p)) return 2;
        if (p.is_identity()) return 1;
        return g1_member(PP::g1_in(p)) ? 1 : 0;
    }
    G16_HD static uint8_t g2_flag(const typename C::G2A& p) {
        if (!PP::g2_on_curve(p)) return 2;
        if (p.is_identity()) return 1;
        return g2_member(PP::g2_in(p)) ? 1 : 0;
    }
};

// a proof's flag from those of its three points: 2 wins over 0, 0 over 1
G16_HD uint8_t subgroup_proof_flag(uint8_t a, uint8_t b, uint8_t c) {
    if (a == 2 || b == 2 || c == 2) return 2;
    return (a == 1 && b == 1 && c == 1) ? 1 : 0;
}

}  // namespace g16
