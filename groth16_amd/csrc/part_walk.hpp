// The bucket-part walk of the bucket pass (msm.hip step 5, MsmPlan::walk == MSM_WALK_PARTS): the layout rule, the task descriptor and
// the per-task walk, written once for the kernel (bucket_parts30_kernel, msm.hip) and for its host twin
// (partslab.hip, g16_host_msm_parts_lab), which runs the same code on the CPU tier and in a sanitizer build.
//
// Layout.  A bucket of n > 0 entries at `off` of the sorted list is cut into np = ceil(n / Lmax) PARTS; part p covers the entries
// [off + p n / np, off + (p + 1) n / np) (integer division): floor(n / np) or ceil(n / np) of them, never more than Lmax, and
// n mod np of the parts are the long ones.  Slot task_off[b] + p holds part p's sum, so a bucket's slot range means what it means
// for the segment walk and the reductions read it unchanged.  One task per slot; a task never crosses a bucket boundary, so the walk
// has no boundary test, no flush and no slot arithmetic inside its loop: it adds its entries and stores the sum once.
#pragma once
#include "fp30.hpp"

namespace g16 {

// one task of the part walk: `len` >= 1 entries of the sorted list from `start`, the sum goes to partial-sum slot `slot`
struct PartTask {
    uint32_t start, len, slot;
};

// parts of a bucket of n entries
G16_HD uint32_t part_count(uint32_t n, uint32_t lmax) { return (uint32_t)(((uint64_t)n + lmax - 1) / lmax); }
// first entry of part p (p <= np) relative to the bucket's offset: floor(p n / np) = p q + floor(p r / np) with n = q np + r;
// floor(p r / np) is also the number of LONG parts (q + 1 entries) among the first p
G16_HD uint32_t part_long_before(uint32_t p, uint32_t r, uint32_t np) { return (uint32_t)((uint64_t)p * r / np); }

// entry word -> position in the table.  Per-window plan: point | sign << 31; merged plan: point | window << 26 | sign << 31, the base
// is table[window][point].  false: the index leaves [0, base_count) after `shift` and the entry is skipped.
G16_HD bool decode_entry(uint32_t v, bool merged, int64_t shift, uint64_t base_count, int64_t* at) {
    const uint32_t pt = merged ? (v & 0x3ffffffu) : (v & 0x7fffffffu);
    const uint64_t row = merged ? (uint64_t)((v >> 26) & 31u) * base_count : 0;
    const int64_t idx = (int64_t)pt + shift;
    *at = (int64_t)row + idx;
    return idx >= 0 && (uint64_t)idx < base_count;
}

// One task: acc (the identity on entry) += the task's entries, then the sum -- raw lazy limbs -- goes to *dst.  The software pipeline
// is the segment walk's: the base of entry i + 1 is gathered, and the word of entry i + 2 loaded, around the addition of entry i
// (before it where F30::ACC_PREFETCH).  `trip` >= task.len is the loop bound -- on the device the largest length in the wave, so that
// the loop's branch is uniform; a lane past its own length idles, which happens only in waves that straddle two length classes.
// The generic `if (inf)` branch of add_affine_core stays: a first entry that is skipped leaves the sum at infinity and the set
// happens on a later entry; in the normal case every lane of the wave sets on entry 0 and adds from entry 1 on.
template <class F30, class Store, class A>
G16_HD void walk_bucket_part(const PartTask& task, uint32_t trip, const uint32_t* __restrict__ sorted, const A* __restrict__ bases, int64_t shift,
                             uint64_t base_count, bool merged, AccParked<F30, Store>& acc, AccRaw<typename F30::Raw>* dst) {
    typedef typename F30::PackedC YNext;   // y stays packed as gathered; it is negated there and unpacked once, when the point is added
    const uint32_t* __restrict__ ent = sorted + task.start;
    const uint32_t len = task.len;
    uint32_t v_next = 0;
    F30 px_next = F30::zero();
    YNext py_next = YNext::zero();
    bool ok_next = false;
    auto fetch = [&](uint32_t v) {
        v_next = v;
        int64_t at = 0;
        ok_next = decode_entry(v, merged, shift, base_count, &at);
        if (ok_next) ok_next = F30::load_point_py(bases, at, px_next, py_next);
    };
    fetch(ent[0]);
    uint32_t v_fetch = 1 < len ? ent[1] : 0u;   // entry i + 1's word, loaded one iteration early
    for (uint32_t i = 0; i < trip; ++i) {
        if (i < len) {
            const uint32_t v = v_next;
            const F30 px = px_next;
            YNext py = py_next;
            const bool ok = ok_next;
            auto advance = [&]() {
                if (i + 1 < len) fetch(v_fetch);
                v_fetch = i + 2 < len ? ent[i + 2] : 0u;
            };
            if constexpr (F30::ACC_PREFETCH) advance();
            if (ok) acc.add_affine_packed(px, py, (v >> 31) != 0);   // the digit's sign and the parked sum's sign are one flip (AccParked)
            if constexpr (!F30::ACC_PREFETCH) advance();
        }
    }
    acc.gather().store_raw(dst);
}

}  // namespace g16
