// R1CS satisfaction on gfx950: is <A_row, z> * <B_row, z> == <C_row, z> for every constraint row, and if not, how many rows fail and
// which is the first.  Restates cs.is_satisfied() / which_is_unsatisfied() (ark-relations), the check the reference makes behind
// debug_assert!(cs.is_satisfied().unwrap()), src/prover.rs:193 -- a debug build panics there, a release build proves the bad witness.
//
// One lane per constraint row, the row walk of the witness maps (csr_row_dot.hpp) three times over: gather-bound like spmv3_kernel,
// one more read of nnz * (32 + 4) bytes + row_ptr + the gathered z.  The instance-copy rows nc .. nc + l of the maps are no constraints
// and are not looked at.  No LDS: a wave reduces with one ballot, one lane of a wave that saw a bad row adds its count and takes the
// minimum of its first bad row on a 16-byte record in HBM.  Count and minimum do not depend on the order the waves arrive in.
#include "internal.hpp"
#include "csr_row_dot.hpp"
#include <new>

namespace g16 {

template <class Fr>
struct CheckArgs {
    const uint64_t* row_ptr[3];
    const uint32_t* col[3];
    const Fr* val[3];
};

// rec[0]: rows that fail (the host zeroes it), rec[1]: the lowest of them (the host sets UINT64_MAX)
template <class Fr>
__global__ __launch_bounds__(256) void r1cs_check_kernel(CheckArgs<Fr> args, const Fr* __restrict__ z, uint32_t nc, unsigned long long* __restrict__ rec) {
    // (a domain has at most 2^30 rows: 32-bit row indices, as in spmv_circom_kernel)
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (row < nc) {
        // a * b is folded before C is walked: one product is alive across each of the later walks, never two sums
        Fr ab = csr_row_dot<Fr>(args.row_ptr[0], args.col[0], args.val[0], z, row);
        ab = ab * csr_row_dot<Fr>(args.row_ptr[1], args.col[1], args.val[1], z, row);
        // operator+ and operator* keep Fr canonical: limb-wise equality is equality in the field
        bad = ab != csr_row_dot<Fr>(args.row_ptr[2], args.col[2], args.val[2], z, row);
    }
    const unsigned long long m = __ballot(bad);   // wave64: one bit per lane, rows ascend with the lane
    if (m == 0) return;
    if ((threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m) - 1)) {   // the wave's first bad row speaks for the wave
        atomicAdd(&rec[0], (unsigned long long)__popcll(m));
        atomicMin(&rec[1], (unsigned long long)row);
    }
}

// out[0..2] = <A_row, z>, <B_row, z>, <C_row, z> of one row: what a failure is reported with
template <class Fr>
__global__ void r1cs_row_values_kernel(CheckArgs<Fr> args, const Fr* __restrict__ z, uint64_t row, Fr* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
#pragma unroll 1
    for (int m = 0; m < 3; ++m) out[m] = csr_row_dot<Fr>(args.row_ptr[m], args.col[m], args.val[m], z, row);
}

template <class C>
int r1cs_check_device(const DeviceCircuit<C>* ck, const typename C::Fr* d_z, void* d_scratch, hipStream_t st, g16_check_result* out) {
    typedef typename C::Fr Fr;
    static_assert(sizeof(Fr) == 32 && 16 + 3 * sizeof(Fr) <= R1CS_CHECK_SCRATCH, "record + three values fit the scratch");
    memset(out, 0, sizeof(*out));
    out->first_row = UINT64_MAX;
    const uint64_t nc = ck->num_constraints;
    if (nc == 0) return G16_OK;
    if (nc >= ((uint64_t)1 << 32) || !ck->row_ptr[2] || ck->long_rows) return G16_ERR_BAD_ARG;
    CheckArgs<Fr> args;
    for (int m = 0; m < 3; ++m) {
        args.row_ptr[m] = ck->row_ptr[m];
        args.col[m] = ck->col[m];
        args.val[m] = ck->val[m];
    }
    unsigned long long* rec = static_cast<unsigned long long*>(d_scratch);
    Fr* vals = reinterpret_cast<Fr*>(static_cast<char*>(d_scratch) + 16);
    G16_HIP_TRY(hipMemsetAsync(rec, 0, 8, st));
    G16_HIP_TRY(hipMemsetAsync(rec + 1, 0xff, 8, st));
    hipLaunchKernelGGL((r1cs_check_kernel<Fr>), dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, args, d_z, (uint32_t)nc, rec);
    G16_LAUNCH_CHECK();
    unsigned long long host_rec[2] = {0, 0};
    G16_HIP_TRY(hipMemcpyAsync(host_rec, rec, 16, hipMemcpyDeviceToHost, st));
    G16_HIP_TRY(hipStreamSynchronize(st));
    out->n_unsatisfied = host_rec[0];
    out->first_row = host_rec[1];
    if (host_rec[0] == 0) return G16_OK;
    if (host_rec[1] >= nc) return G16_ERR_INTERNAL;   // a count without a row: the record was not the kernel's
    hipLaunchKernelGGL((r1cs_row_values_kernel<Fr>), dim3(1), dim3(64), 0, st, args, d_z, (uint64_t)host_rec[1], vals);
    G16_LAUNCH_CHECK();
    Fr host_vals[3];
    G16_HIP_TRY(hipMemcpyAsync(host_vals, vals, sizeof(host_vals), hipMemcpyDeviceToHost, st));
    G16_HIP_TRY(hipStreamSynchronize(st));
    memcpy(out->a, &host_vals[0], 32);
    memcpy(out->b, &host_vals[1], 32);
    memcpy(out->c, &host_vals[2], 32);
    return G16_OK;
}

template <class C>
int r1cs_attach_c_device(DeviceCircuit<C>* ck, const g16_csr_view* c, hipStream_t st) {
    typedef typename C::Fr Fr;
    const uint64_t nc = ck->num_constraints, nnz = c->row_ptr[nc];
    uint64_t* d_rp = nullptr;
    uint32_t* d_col = nullptr;
    Fr* d_val = nullptr;
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(d_rp); (void)hipFree(d_col); (void)hipFree(d_val);
        return code;
    };
    if (hipMalloc((void**)&d_rp, (nc + 1) * sizeof(uint64_t)) != hipSuccess) return fail(G16_ERR_OOM);
    if (hipMalloc((void**)&d_col, (nnz ? nnz : 1) * sizeof(uint32_t)) != hipSuccess) return fail(G16_ERR_OOM);
    if (hipMalloc((void**)&d_val, (nnz ? nnz : 1) * sizeof(Fr)) != hipSuccess) return fail(G16_ERR_OOM);
    if (hipMemcpyAsync(d_rp, c->row_ptr, (nc + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st) != hipSuccess) return fail(G16_ERR_HIP);
    if (nnz) {
        if (hipMemcpyAsync(d_col, c->col, nnz * sizeof(uint32_t), hipMemcpyHostToDevice, st) != hipSuccess) return fail(G16_ERR_HIP);
        if (hipMemcpyAsync(d_val, c->val, nnz * sizeof(Fr), hipMemcpyHostToDevice, st) != hipSuccess) return fail(G16_ERR_HIP);
        if (ck->num_variables < (1ull << 31)) {   // as mark_unit_coefficients: only when every index fits 31 bits
            const int rc = mark_unit_matrix<C>(d_col, d_val, nnz, st);
            if (rc) return fail(rc);
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(G16_ERR_HIP);
    ck->row_ptr[2] = d_rp;
    ck->col[2] = d_col;
    ck->val[2] = d_val;
    ck->nnz[2] = nnz;
    return G16_OK;
}

template <class C>
int r1cs_check_host(const g16_csr_view abc[3], uint64_t nc, const uint64_t* z_, uint64_t n_assign, g16_check_result* out) {
    typedef typename C::Fr Fr;
    memset(out, 0, sizeof(*out));
    out->first_row = UINT64_MAX;
    if (nc == 0) return G16_OK;
    for (int m = 0; m < 3; ++m) {   // what g16_circuit_load checks before a kernel may walk the arrays
        if (!abc[m].row_ptr) return G16_ERR_BAD_ARG;
        if (abc[m].row_ptr[0] != 0) return G16_ERR_BAD_LENGTH;
        for (uint64_t i = 0; i < nc; ++i) {
            if (abc[m].row_ptr[i] > abc[m].row_ptr[i + 1]) return G16_ERR_BAD_LENGTH;
            if (abc[m].row_ptr[i + 1] - abc[m].row_ptr[i] >= ((uint64_t)1 << 32)) return G16_ERR_BAD_LENGTH;
        }
        const uint64_t nnz = abc[m].row_ptr[nc];
        if (nnz && (!abc[m].col || !abc[m].val)) return G16_ERR_BAD_ARG;
        for (uint64_t k = 0; k < nnz; ++k)
            if (abc[m].col[k] >= n_assign) return G16_ERR_BAD_LENGTH;
    }
    const Fr* z = reinterpret_cast<const Fr*>(z_);
    auto dot = [&](int m, uint64_t row) {
        return csr_row_dot<Fr, false>(abc[m].row_ptr, abc[m].col, reinterpret_cast<const Fr*>(abc[m].val), z, row);
    };
    for (uint64_t row = 0; row < nc; ++row) {
        const Fr a = dot(0, row), b = dot(1, row), c = dot(2, row);
        if (a * b == c) continue;
        if (out->n_unsatisfied++ == 0) {
            out->first_row = row;
            memcpy(out->a, &a, 32);
            memcpy(out->b, &b, 32);
            memcpy(out->c, &c, 32);
        }
    }
    return G16_OK;
}

#define G16_INSTANTIATE_CHECK(C)                                                                                                       \
    template int r1cs_check_device<C>(const DeviceCircuit<C>*, const typename C::Fr*, void*, hipStream_t, g16_check_result*);          \
    template int r1cs_attach_c_device<C>(DeviceCircuit<C>*, const g16_csr_view*, hipStream_t);                                         \
    template int r1cs_check_host<C>(const g16_csr_view[3], uint64_t, const uint64_t*, uint64_t, g16_check_result*);
G16_INSTANTIATE_CHECK(Bls12_381)
G16_INSTANTIATE_CHECK(Bn254)

}  // namespace g16
