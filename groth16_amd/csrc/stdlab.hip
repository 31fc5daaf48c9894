// The standard-form lab: single operations of field.hpp (Fp<P>, Fp2<P>: 32-bit Montgomery words in arkworks' form) and curve.hpp
// (Affine<F>, XYZZ<F>), one tuple per lane on the device (g16_dev_std_op) and the same function compiled for the host
// (g16_host_std_op).  Test hooks like the tower lab: not on a proof's path.  The device's Montgomery product, Fp::mul_cios32, is what
// every kernel that multiplies standard-form values runs; the host's operator* runs mul_host64 instead, so the product forms exist
// twice: 4 / 5 / 8 through operator* (the device's body on the device, the 64-bit body on the host) and 14 / 15 / 18 through
// mul_cios32 by name on both sides.  One kernel per curve and kind switches on the form (uniform over a launch); its name starts with
// devlab_.  include/g16_mi355x.h lists the forms.
#include "internal.hpp"
#include "curve.hpp"
#include <vector>

using namespace g16;

namespace g16 {
int ctx_devices(const g16_ctx* ctx, int* curve, std::vector<int>& devs, std::vector<hipStream_t>& streams);   // api.hip
}

namespace {

// ---- slots: one base-field element, F::N 32-bit words
template <class F>
struct Slots;
template <class P>
struct Slots<Fp<P>> {
    typedef Fp<P> F;
    typedef F Base;
    static constexpr int C = 1;
    G16_HD static F ld(const uint32_t* s, int k) {
        F r;
        G16_UNROLL for (int i = 0; i < F::N; ++i) r.v[i] = s[k * F::N + i];
        return r;
    }
    G16_HD static void st(uint32_t* o, int k, const F& a) {
        G16_UNROLL for (int i = 0; i < F::N; ++i) o[k * F::N + i] = a.v[i];
    }
};
template <class P>
struct Slots<Fp2<P>> {
    typedef Fp2<P> F;
    typedef Fp<P> Base;
    static constexpr int C = 2;
    G16_HD static F ld(const uint32_t* s, int k) { return {Slots<Base>::ld(s, k), Slots<Base>::ld(s, k + 1)}; }
    G16_HD static void st(uint32_t* o, int k, const F& a) { Slots<Base>::st(o, k, a.c0); Slots<Base>::st(o, k + 1, a.c1); }
};

// operand / output slots of a form; false for an unknown kind or form
constexpr bool std_slots(int kind, int form, int* nin, int* nout) {
    int i = 0, o = 0;
    if (kind == 0 || kind == 1) {
        switch (form) {
            case 0: case 1: case 4: case 14: i = 2; o = 1; break;
            case 2: case 3: case 5: case 6: case 7: case 8: case 15: case 18: i = 1; o = 1; break;
            case 9: i = 2; o = 1; break;
            default: return false;
        }
    } else if (kind == 2) {
        switch (form) {
            case 0: case 1: case 4: i = 4; o = 2; break;
            case 2: case 3: case 5: case 6: i = 2; o = 2; break;
            default: return false;
        }
    } else if (kind == 3 || kind == 4) {
        const int c = kind == 3 ? 1 : 2;
        switch (form) {
            case 0: i = 4 * c; o = 4 * c; break;
            case 1: i = 8 * c; o = 4 * c; break;
            case 2: case 4: i = 4 * c; o = 4 * c; break;
            case 3: i = 2 * c; o = 4 * c; break;
            case 5: i = 4 * c + 2; o = 4 * c; break;
            case 6: i = 4 * c; o = 2 * c; break;
            default: return false;
        }
    } else {
        return false;
    }
    *nin = i;
    *nout = o;
    return true;
}

template <class F>
struct FieldLab {
    typedef Slots<F> S;
    static constexpr int N = F::N;
    __host__ __device__ static void run(int form, const uint32_t* in, uint32_t* out) {
        switch (form) {
            case 0: S::st(out, 0, S::ld(in, 0) + S::ld(in, 1)); break;
            case 1: S::st(out, 0, S::ld(in, 0) - S::ld(in, 1)); break;
            case 2: S::st(out, 0, S::ld(in, 0).neg()); break;
            case 3: S::st(out, 0, S::ld(in, 0).dbl()); break;
            case 4: S::st(out, 0, S::ld(in, 0) * S::ld(in, 1)); break;
            case 5: S::st(out, 0, S::ld(in, 0).sqr()); break;
            case 6: S::st(out, 0, S::ld(in, 0).inverse()); break;
            case 7: {
                F r;
                S::ld(in, 0).to_canonical(r.v);
                S::st(out, 0, r);
                break;
            }
            case 8: S::st(out, 0, F::from_canonical(in)); break;
            case 9: {
                const F a = S::ld(in, 0), b = S::ld(in, 1);
                G16_UNROLL for (int i = 0; i < N; ++i) out[i] = 0;
                out[0] = a.is_zero() ? 1u : 0u;
                out[1] = a.is_one() ? 1u : 0u;
                out[2] = a == b ? 1u : 0u;
                break;
            }
            // the device's product by name
            case 14: S::st(out, 0, S::ld(in, 0).mul_cios32(S::ld(in, 1))); break;
            case 15: { const F a = S::ld(in, 0); S::st(out, 0, a.mul_cios32(a)); break; }
            case 18: S::st(out, 0, S::ld(in, 0).mul_cios32(F::r2())); break;
            default: break;
        }
    }
};

template <class F2>
struct Field2Lab {
    typedef Slots<F2> S;
    static constexpr int N = F2::Base::N;
    __host__ __device__ static void run(int form, const uint32_t* in, uint32_t* out) {
        switch (form) {
            case 0: S::st(out, 0, S::ld(in, 0) + S::ld(in, 2)); break;
            case 1: S::st(out, 0, S::ld(in, 0) - S::ld(in, 2)); break;
            case 2: S::st(out, 0, S::ld(in, 0).neg()); break;
            case 3: S::st(out, 0, S::ld(in, 0).dbl()); break;
            case 4: S::st(out, 0, S::ld(in, 0) * S::ld(in, 2)); break;
            case 5: S::st(out, 0, S::ld(in, 0).sqr()); break;
            case 6: S::st(out, 0, S::ld(in, 0).inverse()); break;
            default: break;
        }
    }
};

template <class F>
struct GroupLab {
    typedef Slots<F> S;
    typedef Affine<F> A;
    typedef XYZZ<F> X;
    static constexpr int N = S::Base::N, C = S::C;
    G16_HD static A ld_aff(const uint32_t* s, int k) { return {S::ld(s, k), S::ld(s, k + C)}; }
    G16_HD static X ld_raw(const uint32_t* s, int k) { return {S::ld(s, k), S::ld(s, k + C), S::ld(s, k + 2 * C), S::ld(s, k + 3 * C)}; }
    G16_HD static void st_raw(uint32_t* o, const X& p) { S::st(o, 0, p.x); S::st(o, C, p.y); S::st(o, 2 * C, p.zz); S::st(o, 3 * C, p.zzz); }
    __host__ __device__ static void run(int form, const uint32_t* in, uint32_t* out) {
        switch (form) {
            case 0: {
                X acc = X::from_affine(ld_aff(in, 0));
                acc.add_affine(ld_aff(in, 2 * C));
                st_raw(out, acc);
                break;
            }
            case 1: {
                X acc = ld_raw(in, 0);
                acc.add(ld_raw(in, 4 * C));
                st_raw(out, acc);
                break;
            }
            case 2: st_raw(out, ld_raw(in, 0).dbl()); break;
            case 3: st_raw(out, X::dbl_affine(ld_aff(in, 0))); break;
            case 4: st_raw(out, ld_raw(in, 0).neg()); break;
            case 5: {
                uint32_t k[8];
                for (int i = 0; i < 8; ++i) k[i] = in[4 * C * N + i];
                const uint32_t nbits = in[(4 * C + 1) * N];
                st_raw(out, ld_raw(in, 0).mul_bits(k, nbits > 256u ? 256 : (int)nbits));
                break;
            }
            case 6: {
                const A r = ld_raw(in, 0).to_affine();
                S::st(out, 0, r.x);
                S::st(out, C, r.y);
                break;
            }
            default: break;
        }
    }
};

template <class C, int KIND>
struct KindLab;
template <class C> struct KindLab<C, 0> : FieldLab<typename C::Fr> {};
template <class C> struct KindLab<C, 1> : FieldLab<typename C::Fq> {};
template <class C> struct KindLab<C, 2> : Field2Lab<typename C::Fq2> {};
template <class C> struct KindLab<C, 3> : GroupLab<typename C::Fq> {};
template <class C> struct KindLab<C, 4> : GroupLab<typename C::Fq2> {};

constexpr int LAB_WG = 64;   // one wavefront per workgroup: 65 tuples already span two workgroups

template <class C, int KIND>
__global__ void __launch_bounds__(LAB_WG) devlab_std_op(int form, int nin, int nout, const uint32_t* __restrict__ in,
                                                        uint32_t* __restrict__ out, uint32_t n) {
    constexpr int N = KindLab<C, KIND>::N;
    const uint32_t t = blockIdx.x * LAB_WG + threadIdx.x;
    if (t >= n) return;
    KindLab<C, KIND>::run(form, in + (size_t)t * nin * N, out + (size_t)t * nout * N);
}

template <class C, int KIND>
int std_device(hipStream_t st, int form, int nin, int nout, const uint32_t* operands, uint64_t n, uint32_t* out) {
    constexpr int N = KindLab<C, KIND>::N;
    const size_t in_bytes = (size_t)n * nin * N * 4, out_bytes = (size_t)n * nout * N * 4;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    G16_HIP_TRY(hipMalloc((void**)&d_in, in_bytes));
    if (hipMalloc((void**)&d_out, out_bytes) != hipSuccess) { (void)hipFree(d_in); return G16_ERR_OOM; }
    auto body = [&]() -> int {
        G16_HIP_TRY(hipMemcpyAsync(d_in, operands, in_bytes, hipMemcpyHostToDevice, st));
        G16_HIP_TRY(hipMemsetAsync(d_out, 0, out_bytes, st));
        devlab_std_op<C, KIND><<<dim3((unsigned)((n + LAB_WG - 1) / LAB_WG)), dim3(LAB_WG), 0, st>>>(form, nin, nout, d_in, d_out, (uint32_t)n);
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

template <class C, int KIND>
int std_any(bool device, hipStream_t st, int form, int nin, int nout, const uint32_t* operands, uint64_t n, uint32_t* out) {
    if (device) return std_device<C, KIND>(st, form, nin, nout, operands, n, out);
    constexpr int N = KindLab<C, KIND>::N;
    for (uint64_t i = 0; i < n; ++i) KindLab<C, KIND>::run(form, operands + i * nin * N, out + i * nout * N);
    return G16_OK;
}

template <class C>
int std_kind(int kind, bool device, hipStream_t st, int form, int nin, int nout, const uint32_t* operands, uint64_t n, uint32_t* out) {
    switch (kind) {
        case 0: return std_any<C, 0>(device, st, form, nin, nout, operands, n, out);
        case 1: return std_any<C, 1>(device, st, form, nin, nout, operands, n, out);
        case 2: return std_any<C, 2>(device, st, form, nin, nout, operands, n, out);
        case 3: return std_any<C, 3>(device, st, form, nin, nout, operands, n, out);
        case 4: return std_any<C, 4>(device, st, form, nin, nout, operands, n, out);
        default: return G16_ERR_BAD_ARG;
    }
}

int std_run(int curve, int kind, bool device, hipStream_t st, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    int nin = 0, nout = 0;
    if (!operands || !out || n == 0 || n > ((uint64_t)1 << 22) || !std_slots(kind, form, &nin, &nout)) return G16_ERR_BAD_ARG;
    if (curve == G16_BLS12_381) return std_kind<Bls12_381>(kind, device, st, form, nin, nout, operands, n, out);
    if (curve == G16_BN254) return std_kind<Bn254>(kind, device, st, form, nin, nout, operands, n, out);
    return G16_ERR_BAD_ARG;
}

}  // namespace

extern "C" int g16_dev_std_op(g16_ctx* ctx, int kind, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    int curve = 0;
    std::vector<int> devs;
    std::vector<hipStream_t> streams;
    G16_TRY(ctx_devices(ctx, &curve, devs, streams));
    G16_HIP_TRY(hipSetDevice(devs[0]));
    return std_run(curve, kind, true, streams[0], form, operands, n, out);
}

extern "C" int g16_host_std_op(int curve, int kind, int form, const uint32_t* operands, uint64_t n, uint32_t* out) {
    return std_run(curve, kind, false, nullptr, form, operands, n, out);
}
