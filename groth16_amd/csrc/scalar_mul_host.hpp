// The task of scalar_mul.hpp on the host, lane by lane (the `not gpu` tests of libg16_phase1.so and libg16_lagrange.so): G1 on Fp30, G2
// on the two components of a lane pair (Fp2h30: each half runs the pair's own product and inversion steps), and the IO of a task
// whose data sits in plain members.  Host code only.
#pragma once
#include "scalar_mul.hpp"

namespace g16 {

template <class P>
struct Fp2h30 {
    typedef Fp30<P> B;
    typedef Fp2p30<P> PP;
    B c0, c1;
    static constexpr int KM = PP::KM, K2M = PP::K2M, KX = PP::KX, KY = PP::KY;
    static Fp2h30 zero() { return {B::zero(), B::zero()}; }
    static Fp2h30 one() { return {B::one(), B::zero()}; }
    Fp2h30 add(const Fp2h30& o) const { return {c0.add(o.c0), c1.add(o.c1)}; }
    Fp2h30 dbl() const { return {c0.dbl(), c1.dbl()}; }
    Fp2h30 add_dbl(const Fp2h30& o) const { return {c0.add_dbl(o.c0), c1.add_dbl(o.c1)}; }
    template <int K> Fp2h30 sub(const Fp2h30& o) const { return {c0.template sub<K>(o.c0), c1.template sub<K>(o.c1)}; }
    Fp2h30 mul(const Fp2h30& o) const { return {PP::pair_mul(false, c0, c1, o.c0, o.c1), PP::pair_mul(true, c1, c0, o.c1, o.c0)}; }
    Fp2h30 sqr() const { return {PP::pair_sqr(false, c0, c1), PP::pair_sqr(true, c1, c0)}; }
    template <int K> Fp2h30 mul_sub_k(const Fp2h30& o, const Fp2h30& s) const { return mul(o).template sub<K>(s); }
    Fp2h30 sqr_sub_x3(const Fp2h30& u, const Fp2h30& v) const { return sqr().template sub<KM + K2M>(u.add_dbl(v)); }
    static Fp2h30 mul_sub(const Fp2h30& a, const Fp2h30& b, const Fp2h30& c, const Fp2h30& d) { return a.mul(b).template sub<KM>(c.mul(d)); }
};
template <class P>
Fp2h30<P> batch_inverse(const Fp2h30<P>& a) { return {pair_inverse<P>(false, a.c0, a.c1), pair_inverse<P>(true, a.c1, a.c0)}; }

template <class P> bool zero30(const Fp30<P>& v) { return v.maybe_zero() && v.is_zero_exact(); }
template <class P> bool zero30(const Fp2h30<P>& v) { return zero30(v.c0) && zero30(v.c1); }

template <class F>
struct SmulHostIO {
    F x0, y0, ox, oy;
    bool finite, oid = true;
    uint32_t kb[SMUL_KWORDS];
    F slots[SMUL_SLOTS];
    bool load(F& x, F& y) const { x = x0; y = y0; return finite; }
    uint32_t kword(int w) const { return kb[w]; }
    void put(int s, const F& v) { slots[s] = v; }
    F get(int s) const { return slots[s]; }
    bool any(bool v) const { return v; }
    bool is_zero(const F& v) const { return zero30(v); }
    F select(bool c, const F& a, const F& b) const { return c ? a : b; }
    void store(const F& x, const F& y, bool identity) { ox = x; oy = y; oid = identity; }
};

template <class P> Fp30<P> in30(const Fp<P>& v) { return Fp30<P>::unpack(Fp30<P>::std_to_r30(v).v); }

}  // namespace g16
