// The tower lab: single operations of the pairing tower (pairing.hpp: Q30, T2 / T6 / T12, the projective line steps, the Frobenius
// maps, Granger-Scott squaring, cyc_pow / cyc_pow_bits, final_exp) on raw limbs, one tuple per lane on the device
// (g16_dev_pairing_op) and the same function compiled for the host (g16_host_pairing_op).  Test hooks like the field lab of
// devtest.hip: not on a verification's path.  Field operands are loaded straight into Q30::a, so any representative below 2 p can be
// fed, and results leave as the raw limbs the operation produced: what the next operation of a chain would see.
// One kernel per curve switches on the form (uniform over a launch) and calls the tower's own out-of-line routines; its name
// starts with devlab_: no resource budget applies to it.  include/g16_mi355x.h lists the forms.
#include "internal.hpp"
#include "pairing.hpp"
#include <vector>

using namespace g16;

namespace g16 {
int ctx_devices(const g16_ctx* ctx, int* curve, std::vector<int>& devs, std::vector<hipStream_t>& streams);   // api.hip
}

namespace {

// operand / output slots of a form (a slot is NL 32-bit words); false for an unknown form
constexpr bool tower_slots(int form, int* nin, int* nout) {
    int i = 0, o = 0;
    switch (form) {
        case 0: case 1: case 4: i = 2; o = 1; break;
        case 2: case 3: case 5: case 6: case 8: case 9: i = 1; o = 1; break;
        case 7: i = 2; o = 1; break;
        case 10: case 11: case 16: i = 4; o = 2; break;
        case 12: case 13: case 14: case 17: case 18: case 19: i = 2; o = 2; break;
        case 15: i = 3; o = 2; break;
        case 20: i = 4; o = 1; break;
        case 30: case 31: case 33: i = 12; o = 6; break;
        case 32: case 34: case 35: i = 6; o = 6; break;
        case 40: i = 24; o = 12; break;
        case 41: case 42: case 43: case 44: i = 12; o = 12; break;
        case 45: i = 12; o = 1; break;
        case 50: i = 13; o = 12; break;
        case 51: i = 24; o = 1; break;
        case 52: case 53: i = 12; o = 12; break;
        case 54: i = 20; o = 12; break;
        case 55: i = 6; o = 12; break;
        case 56: i = 10; o = 12; break;
        case 57: i = 5; o = 4; break;
        case 58: case 59: i = 13; o = 12; break;
        case 60: i = 12; o = 12; break;
        case 61: i = 12; o = 13; break;
        case 62: i = 2; o = 1; break;
        case 63: i = 4; o = 1; break;
        default: return false;
    }
    *nin = i;
    *nout = o;
    return true;
}

template <class C>
struct TowerLab {
    typedef Pairing<C> PP;
    typedef typename PP::P P;
    typedef typename PP::F F;
    typedef typename PP::F2 F2;
    typedef typename PP::F6 F6;
    typedef typename PP::F12 F12;
    typedef typename C::Fq Fq;
    static constexpr int NL = Fp30<P>::NL, XI = PP::XI;

    // ---- slots: raw limbs, the standard form's words, a flag
    G16_HD static F ld1(const uint32_t* s, int k) {
        F r;
        G16_UNROLL for (int i = 0; i < NL; ++i) r.a.l[i] = s[k * NL + i];
        return r;
    }
    G16_HD static F2 ld2(const uint32_t* s, int k) { return {ld1(s, k), ld1(s, k + 1)}; }
    G16_HD static F6 ld6(const uint32_t* s, int k) { return {ld2(s, k), ld2(s, k + 2), ld2(s, k + 4)}; }
    G16_HD static F12 ld12(const uint32_t* s, int k) { return {ld6(s, k), ld6(s, k + 6)}; }
    G16_HD static void st1(uint32_t* o, int k, const F& v) {
        G16_UNROLL for (int i = 0; i < NL; ++i) o[k * NL + i] = v.a.l[i];
    }
    G16_HD static void st2(uint32_t* o, int k, const F2& v) { st1(o, k, v.c0); st1(o, k + 1, v.c1); }
    G16_HD static void st6(uint32_t* o, int k, const F6& v) { st2(o, k, v.c0); st2(o, k + 2, v.c1); st2(o, k + 4, v.c2); }
    G16_HD static void st12(uint32_t* o, int k, const F12& v) { st6(o, k, v.c0); st6(o, k + 6, v.c1); }
    G16_HD static void st_flag(uint32_t* o, int k, bool b) {
        G16_UNROLL for (int i = 0; i < NL; ++i) o[k * NL + i] = (i == 0 && b) ? 1u : 0u;
    }
    G16_HD static Fq ld_words(const uint32_t* s, int k) {
        Fq r;
        G16_UNROLL for (int i = 0; i < Fq::N; ++i) r.v[i] = s[k * NL + i];
        return r;
    }
    G16_HD static void st_words(uint32_t* o, int k, const Fq& v) {
        G16_UNROLL for (int i = 0; i < NL; ++i) o[k * NL + i] = i < Fq::N ? v.v[i] : 0u;
    }
    // a GT value in arkworks' form (12 Fq, Fq::N / 2 64-bit limbs each) <-> 12 slots of 32-bit words
    G16_HD static void st_gt(uint32_t* o, const uint64_t* gt) {
        constexpr int L = Fq::N / 2;
        for (int c = 0; c < 12; ++c)
            for (int i = 0; i < NL; ++i) o[c * NL + i] = i < Fq::N ? (uint32_t)(gt[c * L + (i >> 1)] >> (32 * (i & 1))) : 0u;
    }

    // one tuple
    __host__ __device__ static void run(int form, const uint32_t* in, uint32_t* out) {
        switch (form) {
            // ---- Q30
            case 0: st1(out, 0, ld1(in, 0) + ld1(in, 1)); break;
            case 1: st1(out, 0, ld1(in, 0) - ld1(in, 1)); break;
            case 2: st1(out, 0, ld1(in, 0).neg()); break;
            case 3: st1(out, 0, ld1(in, 0).dbl()); break;
            case 4: st1(out, 0, ld1(in, 0) * ld1(in, 1)); break;
            case 5: st1(out, 0, ld1(in, 0).sqr()); break;
            case 6: st_flag(out, 0, ld1(in, 0).is_zero()); break;
            case 7: st_flag(out, 0, ld1(in, 0) == ld1(in, 1)); break;
            case 8: st1(out, 0, ld1(in, 0).inverse()); break;
            case 9: st_words(out, 0, F::from_std(ld_words(in, 0)).to_std()); break;
            // ---- T2
            case 10: st2(out, 0, ld2(in, 0) + ld2(in, 2)); break;
            case 11: st2(out, 0, ld2(in, 0) - ld2(in, 2)); break;
            case 12: st2(out, 0, ld2(in, 0).neg()); break;
            case 13: st2(out, 0, ld2(in, 0).conj()); break;
            case 14: st2(out, 0, ld2(in, 0).dbl()); break;
            case 15: st2(out, 0, ld2(in, 0).scale(ld1(in, 2))); break;
            case 16: st2(out, 0, F2::mul_outlined(ld2(in, 0), ld2(in, 2))); break;
            case 17: st2(out, 0, F2::sqr_outlined(ld2(in, 0))); break;
            case 18: st2(out, 0, ld2(in, 0).inverse()); break;
            case 19: st2(out, 0, mul_by_xi<F, XI>(ld2(in, 0))); break;
            case 20: st_flag(out, 0, ld2(in, 0) == ld2(in, 2)); break;
            // ---- T6
            case 30: st6(out, 0, ld6(in, 0) + ld6(in, 6)); break;
            case 31: st6(out, 0, ld6(in, 0) - ld6(in, 6)); break;
            case 32: st6(out, 0, ld6(in, 0).neg()); break;
            case 33: st6(out, 0, F6::mul_outlined(ld6(in, 0), ld6(in, 6))); break;
            case 34: st6(out, 0, ld6(in, 0).mul_by_v()); break;
            case 35: st6(out, 0, ld6(in, 0).inverse()); break;
            // ---- T12
            case 40: st12(out, 0, F12::mul_outlined(ld12(in, 0), ld12(in, 12))); break;
            case 41: st12(out, 0, F12::sqr_outlined(ld12(in, 0))); break;
            case 42: st12(out, 0, F12::cyc_sqr_outlined(ld12(in, 0))); break;
            case 43: st12(out, 0, ld12(in, 0).conj()); break;
            case 44: st12(out, 0, ld12(in, 0).inverse()); break;
            case 45: st_flag(out, 0, ld12(in, 0).is_zero()); break;
            // ---- Pairing<C>
            case 50: {
                const uint32_t j = in[12 * NL];
                st12(out, 0, PP::frob(ld12(in, 0), j < 1u ? 1 : j > 3u ? 3 : (int)j));
                break;
            }
            case 51: st_flag(out, 0, PP::equal(ld12(in, 0), ld12(in, 12))); break;
            case 52: {
                uint64_t gt[12 * (Fq::N / 2)];
                PP::store_gt(ld12(in, 0), gt);
                st_gt(out, gt);
                break;
            }
            case 53: {
                constexpr int L = Fq::N / 2;
                uint64_t gt[12 * L], back[12 * L];
                for (int c = 0; c < 12; ++c)
                    for (int w = 0; w < L; ++w) gt[c * L + w] = (uint64_t)in[c * NL + 2 * w] | ((uint64_t)in[c * NL + 2 * w + 1] << 32);
                PP::store_gt(PP::load_gt(gt), back);
                st_gt(out, back);
                break;
            }
            case 54: {
                F12 f = ld12(in, 0);
                PP::ell(f, typename PP::Ell{ld2(in, 12), ld2(in, 14), ld2(in, 16)}, typename PP::A1{ld1(in, 18), ld1(in, 19)});
                st12(out, 0, f);
                break;
            }
            case 55: case 56: {
                typename PP::Proj t = {ld2(in, 0), ld2(in, 2), ld2(in, 4)};
                const typename PP::Ell e = form == 55 ? PP::Proj::dbl_step(t) : PP::Proj::add_step(t, typename PP::A2{ld2(in, 6), ld2(in, 8)});
                st2(out, 0, t.x); st2(out, 2, t.y); st2(out, 4, t.z);
                st2(out, 6, e.c0); st2(out, 8, e.c1); st2(out, 10, e.c2);
                break;
            }
            case 57: {
                const typename PP::A2 r = PP::frob_twist(typename PP::A2{ld2(in, 0), ld2(in, 2)}, in[4 * NL] == 2u ? 2 : 1);
                st2(out, 0, r.x); st2(out, 2, r.y);
                break;
            }
            case 58: {
                const uint64_t e = (uint64_t)in[12 * NL] | ((uint64_t)in[12 * NL + 1] << 32);
                st12(out, 0, PP::cyc_pow(ld12(in, 0), e ? e : 1u));   // (cyc_pow is defined for e > 0)
                break;
            }
            case 59: {
                uint32_t e[8];
                for (int i = 0; i < 8; ++i) e[i] = in[12 * NL + i];
                const uint32_t nbits = in[12 * NL + 8];
                st12(out, 0, PP::cyc_pow_bits(ld12(in, 0), e, nbits > 256u ? 256 : (int)nbits));
                break;
            }
            case 60: st12(out, 0, PP::exp_by_x(ld12(in, 0))); break;
            case 61: {
                F12 e = {F6::zero(), F6::zero()};
                const bool ok = PP::final_exp(ld12(in, 0), e);
                if (!ok) e = {F6::zero(), F6::zero()};
                st12(out, 0, e);
                st_flag(out, 12, ok);
                break;
            }
            case 62: st_flag(out, 0, PP::g1_on_curve(typename C::G1A{ld_words(in, 0), ld_words(in, 1)})); break;
            case 63:
                st_flag(out, 0, PP::g2_on_curve(typename C::G2A{typename C::Fq2{ld_words(in, 0), ld_words(in, 1)},
                                                                 typename C::Fq2{ld_words(in, 2), ld_words(in, 3)}}));
                break;
            default: break;
        }
    }
};

constexpr int LAB_WG = 64;   // one wavefront per workgroup: 65 tuples already span two workgroups

template <class C>
__global__ void __launch_bounds__(LAB_WG) devlab_tower_op(int form, int nin, int nout, const uint32_t* __restrict__ in,
                                                          uint32_t* __restrict__ out, uint32_t n) {
    constexpr int NL = TowerLab<C>::NL;
    const uint32_t t = blockIdx.x * LAB_WG + threadIdx.x;
    if (t >= n) return;
    TowerLab<C>::run(form, in + (size_t)t * nin * NL, out + (size_t)t * nout * NL);
}

template <class C>
int tower_device(hipStream_t st, int form, int nin, int nout, const uint32_t* operands, uint64_t n, uint32_t* out) {
    constexpr int NL = TowerLab<C>::NL;
    const size_t in_bytes = (size_t)n * nin * NL * 4, out_bytes = (size_t)n * nout * NL * 4;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    G16_HIP_TRY(hipMalloc((void**)&d_in, in_bytes));
    if (hipMalloc((void**)&d_out, out_bytes) != hipSuccess) { (void)hipFree(d_in); return G16_ERR_OOM; }
    auto body = [&]() -> int {
        G16_HIP_TRY(hipMemcpyAsync(d_in, operands, in_bytes, hipMemcpyHostToDevice, st));
        G16_HIP_TRY(hipMemsetAsync(d_out, 0, out_bytes, st));
        devlab_tower_op<C><<<dim3((unsigned)((n + LAB_WG - 1) / LAB_WG)), dim3(LAB_WG), 0, st>>>(form, nin, nout, d_in, d_out, (uint32_t)n);
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

template <class C>
int tower_any(bool device, hipStream_t st, int form, int nin, int nout, const uint32_t* operands, uint64_t n, uint32_t* out) {
    if (device) return tower_device<C>(st, form, nin, nout, operands, n, out);
    constexpr int NL = TowerLab<C>::NL;
    for (uint64_t i = 0; i < n; ++i) TowerLab<C>::run(form, operands + i * nin * NL, out + i * nout * NL);
    return G16_OK;
}

int tower_run(int curve, bool device, hipStream_t st, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    int nin = 0, nout = 0;
    if (!operands || !out || n == 0 || n > ((uint64_t)1 << 22) || !tower_slots(form, &nin, &nout)) return G16_ERR_BAD_ARG;
    if (curve == G16_BLS12_381) return tower_any<Bls12_381>(device, st, form, nin, nout, operands, n, out);
    if (curve == G16_BN254) return tower_any<Bn254>(device, st, form, nin, nout, operands, n, out);
    return G16_ERR_BAD_ARG;
}

}  // namespace

extern "C" int g16_dev_pairing_op(g16_ctx* ctx, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    int curve = 0;
    std::vector<int> devs;
    std::vector<hipStream_t> streams;
    G16_TRY(ctx_devices(ctx, &curve, devs, streams));
    G16_HIP_TRY(hipSetDevice(devs[0]));
    return tower_run(curve, true, streams[0], form, operands, n, out);
}

extern "C" int g16_host_pairing_op(int curve, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    return tower_run(curve, false, nullptr, form, operands, n, out);
}
