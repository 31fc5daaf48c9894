// The argument block of a batched bucket pass (msm.hip step 5), shared by bucket_accumulate30_kernel (msm.hip) and the part walk's
// bucket_parts30_kernel (partwalk.hip).
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
// bucket_parts30_kernel over a host upper bound of `max_tasks` tasks per MSM for the n MSMs of the batch (slot_off[M] is the real count,
// read on the device; surplus lanes exit); lds_pad: unused dynamic LDS (msm.hip pass_lds_pad).  F30 = Fp30<P> or Fp2p30<P> of either curve.
template <class F30>
int msm_parts_pass_launch(const PassBatch<F30>& batch, const PartTaskBatch& tasks, int n, uint32_t max_tasks, uint32_t M, bool merged,
                          unsigned lds_pad, hipStream_t st);

}  // namespace g16
