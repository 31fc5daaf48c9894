// The input-preparation lab: the verifier's prepared input IC = gamma_abc_g1[0] + sum_j x_j gamma_abc_g1[j + 1] in place.
//   g16_dev_pvk_tables       a prepared key's resident window tables (verify_window_table_kernel's output), copied back
//   g16_dev_prepare_inputs   one lane per row of inputs: prepare_inputs_tab on the key's resident tables and gabc0, as
//                            verify_batch_kernel calls it, with the point written out where that kernel goes on to the Miller loop
//   g16_host_pvk_tables, g16_host_prepare_inputs   the same two on the CPU: the tables built by window_table_entry, the text the
//                            table kernel runs, then the same prepare_inputs_tab
// Test hooks like the tower lab: not on a verification's path.  The kernel's name starts with devlab_: no resource budget applies
// to it.  Points leave in the ABI's G1 affine form (standard Montgomery words, the identity all-zero).
#include "verify_common.hpp"
#include <thread>

using namespace g16;

namespace {

constexpr int LAB_WG = 64;   // one wavefront per workgroup, as verify_batch_kernel: 65 rows already span two workgroups

template <class C>
G16_HD typename C::G1A aff_out(const Aff1<C>& p) {
    typename C::G1A o = C::G1A::identity();
    if (!p.is_identity()) { o.x = p.x.to_std(); o.y = p.y.to_std(); }
    return o;
}

template <class C>
__global__ void __launch_bounds__(LAB_WG) devlab_prepare_inputs(const typename C::G1A* gabc0, const Aff1<C>* tables, const uint64_t* inputs,
                                                                uint64_t num_public, uint64_t n, typename C::G1A* out) {
    const uint64_t i = (uint64_t)blockIdx.x * LAB_WG + threadIdx.x;
    if (i >= n) return;
    out[i] = aff_out<C>(prepare_inputs_tab<C>(*gabc0, tables, reinterpret_cast<const typename C::Fr*>(inputs) + i * num_public, num_public));
}

template <class C>
int dev_pvk_tables(const CtxView& cv, const g16_pvk* pvk, int device_index, uint64_t* out) {
    typedef typename C::G1A G1A;
    const std::vector<PvkDev<C>>& pd = devs_of<C>(const_cast<g16_pvk*>(pvk));
    if (pd.size() != cv.devs.size() || device_index < 0 || (size_t)device_index >= pd.size()) return G16_ERR_BAD_ARG;
    const size_t count = (size_t)(pvk->n_gamma_abc - 1) * WINDOWS * DIGITS;
    if (!count) return G16_OK;
    std::vector<Aff1<C>> raw(count);
    G16_HIP_TRY(hipSetDevice(pd[device_index].device));
    G16_HIP_TRY(hipMemcpy(raw.data(), pd[device_index].tables, count * sizeof(Aff1<C>), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < count; ++t) {
        const G1A p = aff_out<C>(raw[t]);
        memcpy(out + t * C::Fq::N, &p, sizeof(G1A));
    }
    return G16_OK;
}

template <class C>
int dev_prepare_inputs(const CtxView& cv, const g16_pvk* pvk, const uint64_t* inputs, uint64_t num_public, uint64_t n, uint64_t* out) {
    typedef typename C::G1A G1A;
    const std::vector<PvkDev<C>>& pd = devs_of<C>(const_cast<g16_pvk*>(pvk));
    if (pd.size() != cv.devs.size() || pd.empty()) return G16_ERR_BAD_ARG;   // the key was loaded on another context
    const PvkDev<C>& d = pd[0];
    G16_HIP_TRY(hipSetDevice(d.device));
    hipStream_t s = cv.streams[0];
    DevBufs bufs;
    uint64_t* d_inputs = nullptr;
    G1A* d_out;
    G16_TRY(bufs.get(&d_out, (size_t)n));
    if (num_public) {
        G16_TRY(bufs.get(&d_inputs, (size_t)n * num_public * 4));
        G16_HIP_TRY(hipMemcpyAsync(d_inputs, inputs, (size_t)n * num_public * 4 * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    }
    devlab_prepare_inputs<C><<<(unsigned)((n + LAB_WG - 1) / LAB_WG), LAB_WG, 0, s>>>(d.gabc0, d.tables, d_inputs, num_public, n, d_out);
    G16_LAUNCH_CHECK();
    std::vector<G1A> res((size_t)n);
    G16_HIP_TRY(hipMemcpyAsync(res.data(), d_out, (size_t)n * sizeof(G1A), hipMemcpyDeviceToHost, s));
    G16_HIP_TRY(hipStreamSynchronize(s));
    memcpy(out, res.data(), (size_t)n * sizeof(G1A));
    return G16_OK;
}

// tables[j][w][d - 1] of gamma_abc_g1[1..], entry by entry as the table kernel's lanes make them; the bases are dealt to a few host
// threads (a base takes a fifth of a second on one)
template <class C>
void host_tables(const g16_vk_view* vk, std::vector<Aff1<C>>& tables) {
    const uint64_t nb = vk->n_gamma_abc - 1;
    tables.resize((size_t)nb * WINDOWS * DIGITS);
    const unsigned nt = (unsigned)std::min<uint64_t>(nb, 8);
    auto work = [&](unsigned t) {
        for (uint64_t j = t; j < nb; j += nt) {
            const typename C::G1A b = ld<typename C::G1A>(vk->gamma_abc_g1 + (j + 1) * C::Fq::N);
            for (int w = 0; w < WINDOWS; ++w)
                for (int d = 1; d <= DIGITS; ++d) tables[((size_t)j * WINDOWS + w) * DIGITS + d - 1] = window_table_entry<C>(b, w, d);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work, t);
    if (nt) work(0);
    for (std::thread& th : pool) th.join();
}

template <class C>
int host_pvk_tables(const g16_vk_view* vk, uint64_t* out) {
    std::vector<Aff1<C>> tables;
    host_tables<C>(vk, tables);
    for (size_t t = 0; t < tables.size(); ++t) {
        const typename C::G1A p = aff_out<C>(tables[t]);
        memcpy(out + t * C::Fq::N, &p, sizeof(p));
    }
    return G16_OK;
}

template <class C>
int host_prepare_inputs(const g16_vk_view* vk, const uint64_t* inputs, uint64_t num_public, uint64_t n, uint64_t* out) {
    typedef typename C::Fr Fr;
    std::vector<Aff1<C>> tables;
    host_tables<C>(vk, tables);
    const typename C::G1A gabc0 = ld<typename C::G1A>(vk->gamma_abc_g1);
    std::vector<Fr> x((size_t)num_public);
    for (uint64_t i = 0; i < n; ++i) {
        for (uint64_t j = 0; j < num_public; ++j) x[j] = ld<Fr>(inputs + (i * num_public + j) * 4);
        const typename C::G1A p = aff_out<C>(prepare_inputs_tab<C>(gabc0, tables.data(), x.data(), num_public));
        memcpy(out + i * C::Fq::N, &p, sizeof(p));
    }
    return G16_OK;
}

}  // namespace

extern "C" {

int g16_dev_pvk_tables(g16_ctx* ctx, const g16_pvk* pvk, int device_index, uint64_t* out) {
    if (!ctx || !pvk || (pvk->n_gamma_abc > 1 && !out)) return G16_ERR_BAD_ARG;
    CtxView cv;
    G16_TRY(cv.load(ctx));
    if (cv.curve != pvk->curve) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(pvk->curve, dev_pvk_tables<CC>(cv, pvk, device_index, out));
}

int g16_dev_prepare_inputs(g16_ctx* ctx, const g16_pvk* pvk, const uint64_t* inputs, uint64_t num_public, uint64_t n, uint64_t* out) {
    if (!ctx || !pvk || (n && !out) || (n && num_public && !inputs) || n > ((uint64_t)1 << 22)) return G16_ERR_BAD_ARG;
    if (num_public + 1 != pvk->n_gamma_abc) return G16_ERR_MALFORMED_VK;
    if (!n) return G16_OK;
    CtxView cv;
    G16_TRY(cv.load(ctx));
    if (cv.curve != pvk->curve) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(pvk->curve, dev_prepare_inputs<CC>(cv, pvk, inputs, num_public, n, out));
}

int g16_host_pvk_tables(int curve, const g16_vk_view* vk, uint64_t* out) {
    if (!vk_view_ok(vk) || (vk->n_gamma_abc > 1 && !out)) return G16_ERR_BAD_ARG;
    G16_VERIFY_DISPATCH(curve, host_pvk_tables<CC>(vk, out));
}

int g16_host_prepare_inputs(int curve, const g16_vk_view* vk, const uint64_t* inputs, uint64_t num_public, uint64_t n, uint64_t* out) {
    if (!vk_view_ok(vk) || (n && !out) || (n && num_public && !inputs)) return G16_ERR_BAD_ARG;
    if (curve != G16_BLS12_381 && curve != G16_BN254) return G16_ERR_BAD_ARG;
    if (num_public + 1 != vk->n_gamma_abc) return G16_ERR_MALFORMED_VK;
    if (!n) return G16_OK;
    G16_VERIFY_DISPATCH(curve, host_prepare_inputs<CC>(vk, inputs, num_public, n, out));
}

}  // extern "C"
