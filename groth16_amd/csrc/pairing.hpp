// Optimal-ate pairing of BLS12-381 and BN254, host + device, on the 30-bit Montgomery products of fp30.hpp.
//
// Replaces ark-ec's Bls12 / Bn pairing as ark-groth16's verifier reaches it (/root/reference/src/verifier.rs:13-76 through
// E::multi_miller_loop and E::final_exponentiation).  The tower is arkworks' in-memory one: Fq6 = Fq2[v]/(v^3 - xi),
// Fq12 = Fq6[w]/(w^2 - v), xi = XI + u (1 + u for BLS12-381, 9 + u for BN254), so a GT value leaves as ark's 12 Fq
// coefficients c0.c0.c0, c0.c0.c1, ..., c1.c2.c1.
//
//   Miller loop   several pairs share one f (ark's multi_miller_loop); G2 steps in homogeneous projective coordinates with
//                 the line coefficients of ark's G2Prepared (doubling / addition formulas of eprint 2010/354), so a fixed G2
//                 point's lines can be written to memory once (prepare) and only evaluated at the G1 point afterwards.
//                 BLS12-381: M-type twist (b' = 4 (1 + u)), loop over |x|, f conjugated because x < 0.
//                 BN254: D-type twist (b' = 3 / (9 + u)), loop over the NAF of 6x + 2, then the lines through pi(Q) and
//                 -pi^2(Q).  A pair with an identity point contributes 1.
//   Final exp.    easy part f^((q^6 - 1)(q^2 + 1)): conjugate, one Fq12 inverse, one Frobenius.  Hard part EXACT (no extra
//                 power lambda): BLS12-381 d = (x - 1)^2 / 3 (x + q)(x^2 + q^2 - 1) + 1, BN254 d = l0 + l1 q + l2 q^2 + q^3
//                 with l2 = 6x^2 + 1, l1 = -36x^3 - 18x^2 - 12x + 1, l0 = -36x^3 - 30x^2 - 18x - 2; x-powers on
//                 Granger-Scott cyclotomic squarings.  The result is f^((q^12 - 1) / r) itself.
//
// Field elements are kept below 2p (Q30 below): a product of such inputs is < 1.5p, every addition / subtraction is followed
// by one conditional subtraction of 2p.  The extension products are out of line so that a verification kernel stays a few
// hundred KB of code.
#pragma once
#include "curve.hpp"
#include "fp30.hpp"

namespace g16 {

// Fq on 30-bit limbs, value kept in [0, 2p)
template <class P>
struct Q30 {
    typedef Fp30<P> B;
    typedef P Params;
    B a;
    G16_HD static Q30 zero() { return {B::zero()}; }
    G16_HD static Q30 one() { return {B::one()}; }
    G16_HD static Q30 from_std(const Fp<P>& x) { return {B::unpack(B::std_to_r30(x).v)}; }
    G16_HD Fp<P> to_std() const { return a.to_std(); }
    template <class K>
    G16_HD static Q30 konst(K k) {   // k(i): 30-bit limbs of a Montgomery constant
        Q30 r;
        G16_UNROLL for (int i = 0; i < B::NL; ++i) r.a.l[i] = k(i);
        return r;
    }
    G16_HD Q30 operator+(const Q30& o) const { return {a.add(o.a).template cond_sub<2>()}; }
    G16_HD Q30 operator-(const Q30& o) const { return {a.template sub<2>(o.a).template cond_sub<2>()}; }
    G16_HD Q30 operator*(const Q30& o) const { return {a.mul(o.a)}; }
    G16_HD Q30 sqr() const { return {a.sqr()}; }
    G16_HD Q30 dbl() const { return *this + *this; }
    G16_HD Q30 neg() const { return {B::zero().template sub<2>(a).template cond_sub<2>()}; }
    G16_HD bool is_zero() const { return a.is_zero_exact(); }
    G16_HD bool operator==(const Q30& o) const { return (*this - o).is_zero(); }
    G16_HD bool operator!=(const Q30& o) const { return !(*this == o); }
    G16_HD Q30 inverse() const { return from_std(to_std().inverse()); }
};

template <class F>
struct T2 {   // Fq2 = Fq[u]/(u^2 + 1)
    typedef typename F::B B;
    F c0, c1;
    G16_HD static T2 zero() { return {F::zero(), F::zero()}; }
    G16_HD static T2 one() { return {F::one(), F::zero()}; }
    G16_HD T2 operator+(const T2& o) const { return {c0 + o.c0, c1 + o.c1}; }
    G16_HD T2 operator-(const T2& o) const { return {c0 - o.c0, c1 - o.c1}; }
    G16_HD T2 neg() const { return {c0.neg(), c1.neg()}; }
    G16_HD T2 dbl() const { return {c0.dbl(), c1.dbl()}; }
    G16_HD T2 conj() const { return {c0, c1.neg()}; }
    G16_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    G16_HD bool operator==(const T2& o) const { return c0 == o.c0 && c1 == o.c1; }
    G16_HD bool operator!=(const T2& o) const { return !(*this == o); }
    G16_HD T2 scale(const F& k) const { return {c0 * k, c1 * k}; }
    // two limb-product sweeps under one reduction per component (Fp2x30's product on strict inputs)
    G16_HD_NOINLINE static T2 mul_outlined(const T2& x, const T2& y) {
        const B nb1 = y.c1.a.neg16();
        return {{B::template mul2_cols<uint64_t>(x.c0.a, y.c0.a, x.c1.a, nb1)}, {B::template mul2_cols<uint64_t>(x.c0.a, y.c1.a, x.c1.a, y.c0.a)}};
    }
    G16_HD_NOINLINE static T2 sqr_outlined(const T2& x) { return {(x.c0 + x.c1) * (x.c0 - x.c1), (x.c0 * x.c1).dbl()}; }
    G16_HD T2 operator*(const T2& o) const { return mul_outlined(*this, o); }
    G16_HD T2 sqr() const { return sqr_outlined(*this); }
    G16_HD T2 inverse() const {
        const F n = (c0.sqr() + c1.sqr()).inverse();
        return {c0 * n, (c1 * n).neg()};
    }
};

template <class F, int XI>
G16_HD T2<F> mul_by_xi(const T2<F>& a) {   // (a0 + a1 u)(XI + u) = (XI a0 - a1) + (a0 + XI a1) u
    if constexpr (XI == 1) return {a.c0 - a.c1, a.c0 + a.c1};
    else {
        static_assert(XI == 9, "xi = 1 + u or 9 + u");
        const F e0 = a.c0.dbl().dbl().dbl() + a.c0, e1 = a.c1.dbl().dbl().dbl() + a.c1;
        return {e0 - a.c1, a.c0 + e1};
    }
}

template <class F, int XI>
struct T6 {   // Fq6 = Fq2[v]/(v^3 - xi)
    typedef T2<F> E2;
    E2 c0, c1, c2;
    G16_HD static T6 zero() { return {E2::zero(), E2::zero(), E2::zero()}; }
    G16_HD static T6 one() { return {E2::one(), E2::zero(), E2::zero()}; }
    G16_HD T6 operator+(const T6& o) const { return {c0 + o.c0, c1 + o.c1, c2 + o.c2}; }
    G16_HD T6 operator-(const T6& o) const { return {c0 - o.c0, c1 - o.c1, c2 - o.c2}; }
    G16_HD T6 neg() const { return {c0.neg(), c1.neg(), c2.neg()}; }
    G16_HD bool is_zero() const { return c0.is_zero() && c1.is_zero() && c2.is_zero(); }
    G16_HD T6 mul_by_v() const { return {mul_by_xi<F, XI>(c2), c0, c1}; }
    G16_HD_NOINLINE static T6 mul_outlined(const T6& a, const T6& b) {   // Karatsuba: 6 Fq2 products
        const E2 v0 = a.c0 * b.c0, v1 = a.c1 * b.c1, v2 = a.c2 * b.c2;
        const E2 r0 = mul_by_xi<F, XI>((a.c1 + a.c2) * (b.c1 + b.c2) - v1 - v2) + v0;
        const E2 r1 = (a.c0 + a.c1) * (b.c0 + b.c1) - v0 - v1 + mul_by_xi<F, XI>(v2);
        const E2 r2 = (a.c0 + a.c2) * (b.c0 + b.c2) - v0 - v2 + v1;
        return {r0, r1, r2};
    }
    G16_HD T6 operator*(const T6& o) const { return mul_outlined(*this, o); }
    G16_HD T6 inverse() const {
        const E2 t0 = c0.sqr() - mul_by_xi<F, XI>(c1 * c2);
        const E2 t1 = mul_by_xi<F, XI>(c2.sqr()) - c0 * c1;
        const E2 t2 = c1.sqr() - c0 * c2;
        const E2 n = (c0 * t0 + mul_by_xi<F, XI>(c2 * t1 + c1 * t2)).inverse();
        return {t0 * n, t1 * n, t2 * n};
    }
};

template <class F, int XI>
struct T12 {   // Fq12 = Fq6[w]/(w^2 - v)
    typedef T2<F> E2;
    typedef T6<F, XI> E6;
    E6 c0, c1;
    G16_HD static T12 one() { return {E6::one(), E6::zero()}; }
    G16_HD T12 conj() const { return {c0, c1.neg()}; }
    G16_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    G16_HD_NOINLINE static T12 mul_outlined(const T12& a, const T12& b) {   // Karatsuba: 3 Fq6 products
        const E6 v0 = a.c0 * b.c0, v1 = a.c1 * b.c1;
        return {v0 + v1.mul_by_v(), (a.c0 + a.c1) * (b.c0 + b.c1) - v0 - v1};
    }
    G16_HD_NOINLINE static T12 sqr_outlined(const T12& a) {   // complex squaring: 2 Fq6 products
        const E6 v2 = a.c0 * a.c1;
        const E6 v0 = (a.c0 - a.c1) * (a.c0 - a.c1.mul_by_v()) + v2;
        return {v0 + v2.mul_by_v(), v2 + v2};
    }
    G16_HD T12 operator*(const T12& o) const { return mul_outlined(*this, o); }
    G16_HD T12 sqr() const { return sqr_outlined(*this); }
    // Granger-Scott squaring, valid in the cyclotomic subgroup (after the easy part of the final exponentiation): 9 Fq2 squarings'
    // worth of products where sqr() spends 12 Fq2 products
    G16_HD_NOINLINE static T12 cyc_sqr_outlined(const T12& a) {
        const E2 &r0 = a.c0.c0, &r4 = a.c0.c1, &r3 = a.c0.c2, &r2 = a.c1.c0, &r1 = a.c1.c1, &r5 = a.c1.c2;
        E2 tmp = r0 * r1;
        const E2 t0 = (r0 + r1) * (mul_by_xi<F, XI>(r1) + r0) - tmp - mul_by_xi<F, XI>(tmp), t1 = tmp.dbl();
        tmp = r2 * r3;
        const E2 t2 = (r2 + r3) * (mul_by_xi<F, XI>(r3) + r2) - tmp - mul_by_xi<F, XI>(tmp), t3 = tmp.dbl();
        tmp = r4 * r5;
        const E2 t4 = (r4 + r5) * (mul_by_xi<F, XI>(r5) + r4) - tmp - mul_by_xi<F, XI>(tmp), t5 = tmp.dbl();
        T12 z;
        z.c0.c0 = (t0 - r0).dbl() + t0;   // 3 t0 - 2 z0
        z.c1.c1 = (t1 + r1).dbl() + t1;   // 3 t1 + 2 z1
        tmp = mul_by_xi<F, XI>(t5);
        z.c1.c0 = (r2 + tmp).dbl() + tmp; // 3 xi t5 + 2 z2
        z.c0.c2 = (t4 - r3).dbl() + t4;   // 3 t4 - 2 z3
        z.c0.c1 = (t2 - r4).dbl() + t2;   // 3 t2 - 2 z4
        z.c1.c2 = (r5 + t3).dbl() + t3;   // 3 t3 + 2 z5
        return z;
    }
    G16_HD T12 cyc_sqr() const { return cyc_sqr_outlined(*this); }
    G16_HD T12 inverse() const {
        const E6 t = (c0 * c0 - (c1 * c1).mul_by_v()).inverse();
        return {c0 * t, (c1 * t).neg()};
    }
    // the w^k coefficient (k = 0..5) of the flat view a_0 + a_1 w + ... + a_5 w^5
    G16_HD E2& coef(int k) {
        E6& h = (k & 1) ? c1 : c0;
        return k < 2 ? h.c0 : k < 4 ? h.c1 : h.c2;
    }
    G16_HD const E2& coef(int k) const { return const_cast<T12*>(this)->coef(k); }
};

template <class C>
struct Pairing {
    typedef typename C::Fq::Params P;
    typedef typename C::K K;
    static constexpr int XI = K::XI;
    static constexpr bool M_TWIST = XI == 1;   // BLS12-381: M-type; BN254: D-type
    typedef Q30<P> F;
    typedef T2<F> F2;
    typedef T6<F, XI> F6;
    typedef T12<F, XI> F12;
    typedef typename C::G1A G1A;   // standard (arkworks) form
    typedef typename C::G2A G2A;
    struct A1 { F x, y; };
    struct A2 { F2 x, y; };
    struct Ell { F2 c0, c1, c2; };   // ark's EllCoeff

    // ---- loop shape
    static constexpr int BLS_BITS = 64;   // |x| = 0xd201000000010000 has its top bit at 63
    G16_HD static constexpr int n_coeffs() {
        if constexpr (M_TWIST) {
            int n = 0;
            for (int i = BLS_BITS - 2; i >= 0; --i) n += 1 + (int)((K::ATE_X_ABS >> i) & 1u);
            return n;
        } else {
            int n = 2;
            for (int i = K::ATE_NAF_LEN - 2; i >= 0; --i) n += 1 + (K::ate_naf(i) != 0);
            return n;
        }
    }
    static constexpr int NCOEFF = n_coeffs();
    enum Step { DBL = 0, ADD = 1, SUB = 2, FROB1 = 3, FROB2N = 4 };

    // ---- conversions to / from the arkworks form
    G16_HD static F2 f2_std(const typename C::Fq2& x) { return {F::from_std(x.c0), F::from_std(x.c1)}; }
    G16_HD static A1 g1_in(const G1A& p) { return {F::from_std(p.x), F::from_std(p.y)}; }
    G16_HD static A2 g2_in(const G2A& p) { return {f2_std(p.x), f2_std(p.y)}; }
    G16_HD static F2 gamma(int j, int k) {
        return {F::konst([=](int i) { return K::frob30(j, k, 0, i); }), F::konst([=](int i) { return K::frob30(j, k, 1, i); })};
    }
    G16_HD static F2 twist_b() { return {F::from_std(C::b2().c0), F::from_std(C::b2().c1)}; }
    G16_HD static F two_inv() { return F::konst([](int i) { return K::two_inv30(i); }); }

    // on-curve tests (the identity passes)
    G16_HD static bool g1_on_curve(const G1A& p) {
        if (p.is_identity()) return true;
        const A1 a = g1_in(p);
        return a.y.sqr() == a.x.sqr() * a.x + F::from_std(C::b1());
    }
    G16_HD static bool g2_on_curve(const G2A& p) {
        if (p.is_identity()) return true;
        const A2 a = g2_in(p);
        return a.y.sqr() == a.x.sqr() * a.x + twist_b();
    }

    // ---- G2 in homogeneous projective coordinates, emitting ark's line coefficients
    struct Proj {
        F2 x, y, z;
        G16_HD_NOINLINE static Ell dbl_step(Proj& t) {
            const F hinv = two_inv();
            const F2 a = (t.x * t.y).scale(hinv);
            const F2 b = t.y.sqr(), c = t.z.sqr();
            const F2 e = twist_b() * (c.dbl() + c);
            const F2 f = e.dbl() + e;
            const F2 g = (b + f).scale(hinv);
            const F2 h = (t.y + t.z).sqr() - (b + c);
            const F2 i = e - b, j = t.x.sqr();
            const F2 e2 = e.sqr();
            t.x = a * (b - f);
            t.y = g.sqr() - (e2.dbl() + e2);
            t.z = b * h;
            if constexpr (M_TWIST) return {i, j.dbl() + j, h.neg()};
            else return {h.neg(), j.dbl() + j, i};
        }
        G16_HD_NOINLINE static Ell add_step(Proj& t, const A2& q) {
            const F2 theta = t.y - q.y * t.z, lambda = t.x - q.x * t.z;
            const F2 c = theta.sqr(), d = lambda.sqr();
            const F2 e = lambda * d, f = t.z * c, g = t.x * d;
            const F2 h = e + f - g.dbl();
            t.x = lambda * h;
            t.y = theta * (g - h) - e * t.y;
            t.z = t.z * e;
            const F2 j = theta * q.x - lambda * q.y;
            if constexpr (M_TWIST) return {j, theta.neg(), lambda};
            else return {lambda, theta.neg(), j};
        }
    };
    // pi^k(Q) on the D-type twist: (conj^k(x) gamma[k][2], conj^k(y) gamma[k][3])
    G16_HD static A2 frob_twist(const A2& q, int k) {
        const A2 c = (k & 1) ? A2{q.x.conj(), q.y.conj()} : q;
        return {c.x * gamma(k, 2), c.y * gamma(k, 3)};
    }
    // a G2 point whose lines are computed as the loop goes
    struct LiveQ {
        Proj t;
        A2 q;
        G16_HD void init(const A2& q0) { q = q0; t = {q0.x, q0.y, F2::one()}; }
        G16_HD Ell next(int step) {
            switch (step) {
                case DBL: return Proj::dbl_step(t);
                case ADD: return Proj::add_step(t, q);
                case SUB: return Proj::add_step(t, A2{q.x, q.y.neg()});
                case FROB1: return Proj::add_step(t, frob_twist(q, 1));
                default: { A2 q2 = frob_twist(q, 2); q2.y = q2.y.neg(); return Proj::add_step(t, q2); }
            }
        }
    };
    // ark's G2Prepared: every line coefficient of a fixed Q, in loop order
    G16_HD static void prepare(const A2& q, Ell* out) {
        LiveQ lq;
        lq.init(q);
        int n = 0;
        drive([&](int step) { out[n++] = lq.next(step); }, [](int) {});
    }

    // The loop skeleton shared by the live and the prepared forms: line(step) evaluates every pair's next line, square(first)
    // squares f (skipped on the first iteration, where f = 1).
    template <class Line, class Square>
    G16_HD static void drive(Line&& line, Square&& square) {
        if constexpr (M_TWIST) {
            for (int i = BLS_BITS - 2; i >= 0; --i) {
                square(i == BLS_BITS - 2);
                line(DBL);
                if ((K::ATE_X_ABS >> i) & 1u) line(ADD);
            }
        } else {
            for (int i = K::ATE_NAF_LEN - 1; i >= 1; --i) {
                square(i == K::ATE_NAF_LEN - 1);
                line(DBL);
                const int d = K::ate_naf(i - 1);
                if (d == 1) line(ADD);
                else if (d == -1) line(SUB);
            }
            line(FROB1);
            line(FROB2N);
        }
    }

    // f *= line(P): sparse element 014 (M-type) or 034 (D-type), multiplied as a full Fq12 element
    G16_HD_NOINLINE static void ell(F12& f, const Ell& c, const A1& p) {
        F12 l = {F6::zero(), F6::zero()};
        if constexpr (M_TWIST) {
            l.c0.c0 = c.c0;
            l.c0.c1 = c.c1.scale(p.x);
            l.c1.c1 = c.c2.scale(p.y);
        } else {
            l.c0.c0 = c.c0.scale(p.y);
            l.c1.c0 = c.c1.scale(p.x);
            l.c1.c1 = c.c2;
        }
        f = f * l;
    }

    // ---- multi-Miller loop over n live pairs (identity points skipped)
    G16_HD static F12 miller_live(const G1A* ps, const G2A* qs, int n, LiveQ* scratch, A1* pa, bool* skip) {
        for (int k = 0; k < n; ++k) {
            skip[k] = ps[k].is_identity() || qs[k].is_identity();
            pa[k] = skip[k] ? A1{F::zero(), F::zero()} : g1_in(ps[k]);
            scratch[k].init(skip[k] ? A2{F2::zero(), F2::zero()} : g2_in(qs[k]));
        }
        F12 f = F12::one();
        drive([&](int step) {
                  for (int k = 0; k < n; ++k)
                      if (!skip[k]) { const Ell c = scratch[k].next(step); ell(f, c, pa[k]); }
              },
              [&](bool first) { if (!first) f = f.sqr(); });
        return finish_loop(f);
    }
    G16_HD static F12 finish_loop(const F12& f) {
        if constexpr (M_TWIST) return K::ATE_X_NEG ? f.conj() : f;
        else return f;
    }

    // ---- final exponentiation
    G16_HD static F12 frob(const F12& a, int j) {
        F12 r;
        G16_UNROLL for (int k = 0; k < 6; ++k) {
            const F2 c = (j & 1) ? a.coef(k).conj() : a.coef(k);
            r.coef(k) = k ? c * gamma(j, k) : c;
        }
        return r;
    }
    G16_HD_NOINLINE static F12 cyc_pow(const F12& a, uint64_t e) {   // a^e, e > 0, a in the cyclotomic subgroup
        F12 r = a;
        int top = 63;
        while (!((e >> top) & 1u)) --top;
        for (int i = top - 1; i >= 0; --i) {
            r = r.cyc_sqr();
            if ((e >> i) & 1u) r = r * a;
        }
        return r;
    }
    // a^e for a canonical little-endian exponent of nbits bits (e = 0 gives 1), a in the cyclotomic subgroup
    G16_HD_NOINLINE static F12 cyc_pow_bits(const F12& a, const uint32_t* e, int nbits) {
        F12 r = F12::one();
        bool started = false;
        for (int i = nbits - 1; i >= 0; --i) {
            if (started) r = r.cyc_sqr();
            if ((e[i >> 5] >> (i & 31)) & 1u) {
                r = started ? r * a : a;
                started = true;
            }
        }
        return r;
    }
    G16_HD static F12 exp_by_x(const F12& a) {   // a^x
        const F12 r = cyc_pow(a, K::ATE_X_ABS);
        return K::ATE_X_NEG ? r.conj() : r;
    }
    // false for f = 0 (SynthesisError::UnexpectedIdentity in ark's final_exponentiation)
    G16_HD static bool final_exp(const F12& f, F12& out) {
        if (f.is_zero()) return false;
        F12 t = f.conj() * f.inverse();   // f^(q^6 - 1)
        t = frob(t, 2) * t;               // ^(q^2 + 1)
        if constexpr (M_TWIST) {
            F12 a = cyc_pow(cyc_pow(t, K::HARD_E_HI), 1ull << 32);
            a = cyc_pow(a, 1ull << 32) * cyc_pow(t, K::HARD_E_LO);   // t^((x - 1)^2 / 3)
            const F12 b = exp_by_x(a) * frob(a, 1);                   // ^(x + q)
            const F12 c = exp_by_x(exp_by_x(b)) * frob(b, 2) * b.conj();   // ^(x^2 + q^2 - 1)
            out = c * t;
        } else {
            const F12 a = exp_by_x(t), b = exp_by_x(a), c = exp_by_x(b);   // t^x, t^x^2, t^x^3
            const F12 c36 = cyc_pow(c, 36), b30 = cyc_pow(b, 30), b18 = cyc_pow(b, 18), a18 = cyc_pow(a, 18), a12 = cyc_pow(a, 12);
            const F12 t0 = (c36 * b30 * a18 * t.cyc_sqr()).conj();   // t^l0
            const F12 t1 = (c36 * b18 * a12).conj() * t;             // t^l1
            const F12 t2 = cyc_pow(b, 6) * t;                        // t^l2
            out = t0 * frob(t1, 1) * frob(t2, 2) * frob(t, 3);
        }
        return true;
    }
    // Straight-line, all six Fq2 comparisons evaluated.  Not a loop `eq = eq && a.coef(k) == b.coef(k)`: left rolled on the device,
    // that loop (a per-lane flag carried round it beside the early exits of the zero tests) answered true for values that differ in
    // c0 only, where the host build of the same text answered false -- the tower lab's `equal` form found it.
    G16_HD static bool equal(const F12& a, const F12& b) {
        bool eq = a.c0.c0 == b.c0.c0;
        eq &= a.c0.c1 == b.c0.c1;
        eq &= a.c0.c2 == b.c0.c2;
        eq &= a.c1.c0 == b.c1.c0;
        eq &= a.c1.c1 == b.c1.c1;
        eq &= a.c1.c2 == b.c1.c2;
        return eq;
    }
    // GT value -> 12 Fq in arkworks' order and Montgomery form (Fq::N / 2 64-bit limbs each)
    G16_HD static void store_gt(const F12& a, uint64_t* out) {
        constexpr int L = C::Fq::N / 2;
        const F2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
        for (int i = 0; i < 6; ++i)
            for (int h = 0; h < 2; ++h) {
                const typename C::Fq s = (h ? c[i]->c1 : c[i]->c0).to_std();
                for (int w = 0; w < L; ++w) out[(2 * i + h) * L + w] = (uint64_t)s.v[2 * w] | ((uint64_t)s.v[2 * w + 1] << 32);
            }
    }
    G16_HD static F12 load_gt(const uint64_t* in) {
        constexpr int L = C::Fq::N / 2;
        F12 a;
        F2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
        for (int i = 0; i < 6; ++i)
            for (int h = 0; h < 2; ++h) {
                typename C::Fq s;
                for (int w = 0; w < L; ++w) { s.v[2 * w] = (uint32_t)in[(2 * i + h) * L + w]; s.v[2 * w + 1] = (uint32_t)(in[(2 * i + h) * L + w] >> 32); }
                (h ? c[i]->c1 : c[i]->c0) = F::from_std(s);
            }
        return a;
    }
};

}  // namespace g16
