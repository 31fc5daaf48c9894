// The argument block of a batched bucket pass (msm.hip step 5), shared by bucket_accumulate30_kernel and the part walk's
// bucket_parts30_kernel (both in msm.hip).
#pragma once
#include "curve.hpp"
#include "fp30.hpp"
#include "part_walk.hpp"

namespace g16 {

static constexpr int PASS_BATCH = 4;
template <class F30>
struct PassBatch {
    const Affine<typename F30::Std>* bases[PASS_BATCH];
    int64_t shift[PASS_BATCH];
    uint64_t base_count[PASS_BATCH];
    const uint32_t* sorted[PASS_BATCH];
    const uint32_t* offsets[PASS_BATCH];
    const uint32_t* slot_off[PASS_BATCH];
    AccRaw<typename F30::Raw>* partials[PASS_BATCH];
};
// the task lists of the same MSMs for the bucket-part walk: one descriptor per partial-sum slot, longest first
struct PartTaskBatch {
    const PartTask* tasks[PASS_BATCH];
};

}  // namespace g16
