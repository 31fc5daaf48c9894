// <M_row, z> of one CSR row: the row walk shared by the Circom map (witness_map.hip), the satisfaction check (r1cs_check.hip) and
// the check's host twin.  Restates evaluate_constraint, src/r1cs_to_qap.rs:28-67, with its coeff.is_one() fast path.
#pragma once
#include <cstdint>
#include "hd.hpp"

namespace g16 {

// MARKED: bit 31 of a column index says "this coefficient is one" (mark_unit_coefficients flags the DEVICE copies at load time; the 32
// bytes of such a coefficient are not even read).  A caller's own host arrays are unmarked: MARKED = false reads every bit as index.
template <class Fr, bool MARKED = true>
G16_HD Fr csr_row_dot(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const Fr* __restrict__ val,
                      const Fr* __restrict__ z, uint64_t row) {
    Fr acc = Fr::zero();
    const Fr one = Fr::one();
    // (a row has fewer than 2^32 terms -- g16_circuit_load_qap checks -- so the walk counts in one register)
    const uint64_t b = row_ptr[row];
    const uint32_t len = (uint32_t)(row_ptr[row + 1] - b);
    col += b;
    val += b;
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t c = col[k];
        if (MARKED && (c >> 31)) {
            acc = acc + z[c & 0x7fffffffu];
        } else {
            const Fr coeff = val[k];
            const Fr v = z[c];
            acc = acc + ((coeff == one) ? v : v * coeff);
        }
    }
    return acc;
}

}  // namespace g16
