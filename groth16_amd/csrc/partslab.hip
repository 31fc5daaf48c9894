// The host twin of the bucket-part walk (g16_host_msm_parts_lab; test hook like hosttest.hip, not on a proof's path): the layout rule
// and walk_bucket_part of part_walk.hpp -- the code bucket_parts30_kernel (msm.hip) runs per lane -- compiled
// for the host, G1 on both curves (the lane pair's G2 arithmetic needs its partner lane and is a device form, as in the field lab).
// The accumulator parks in ParkedArrayStore instead of LDS.  A translation unit of its own that takes nothing from the rest of the
// library, so that tests/parts_walk_replay.cpp builds with it alone under -fsanitize=address,undefined: table, sorted list and records
// are exactly sized heap copies here, and an index the walk gets wrong is the sanitizer's to report.
#include "internal.hpp"
#include "fp30.hpp"
#include "part_walk.hpp"
#include <cstring>
#include <vector>

using namespace g16;

namespace {

template <class C>
int parts_lab_host(int merged, int c, int groups, int lmax, int rows, g16_pass_lab_job* job) {
    typedef typename C::Fq Fq;
    typedef Fp30<typename Fq::Params> F30;
    typedef AccRaw<F30> Raw;
    typedef Affine<Fq> A;
    typedef XYZZ<Fq> X;
    static_assert(sizeof(Raw) == 4 * F30::NL * sizeof(uint32_t), "a record is four coordinates of NL limbs");
    if (!job || c < 2 || c > 16 || groups < 1 || groups > 32 || lmax < 8 || lmax > 4096) return G16_ERR_BAD_ARG;
    if (rows < 1 || rows > 32 || (!merged && rows != 1)) return G16_ERR_BAD_ARG;
    const uint32_t B = 1u << (c - 1), M = B * (uint32_t)groups;
    if (M > (1u << 12)) return G16_ERR_BAD_ARG;
    if (!job->counts || !job->records || !job->offsets || !job->task_off || !job->heavy || !job->out_affine) return G16_ERR_BAD_ARG;
    if (job->n_sorted > ((uint64_t)1 << 16) || (job->n_sorted && !job->sorted)) return G16_ERR_BAD_ARG;
    if (job->base_count > ((uint64_t)1 << 16) || (job->base_count && !job->table)) return G16_ERR_BAD_ARG;
    if (job->shift > ((int64_t)1 << 40) || job->shift < -((int64_t)1 << 40)) return G16_ERR_BAD_ARG;
    uint64_t total = 0;
    for (uint32_t b = 0; b < M; ++b) total += job->counts[b];
    if (total != job->n_sorted) return G16_ERR_BAD_ARG;
    if (merged)
        for (uint64_t e = 0; e < job->n_sorted; ++e)
            if (((job->sorted[e] >> 26) & 31u) >= (uint32_t)rows) return G16_ERR_BAD_ARG;
    if (job->record_cap < job->n_sorted / (uint64_t)lmax + M) return G16_ERR_BAD_LENGTH;
    // the table in the bucket pass's radix (what convert_bases leaves), the sorted list: exactly sized
    const size_t npts = (size_t)rows * job->base_count;
    std::vector<A> table(npts);
    for (size_t i = 0; i < npts; ++i) {
        A a;
        memcpy(&a, job->table + i * (sizeof(A) / sizeof(uint64_t)), sizeof(A));
        table[i] = A{F30::std_to_r30(a.x), F30::std_to_r30(a.y)};   // 0 stays 0: the identity encoding (0, 0) is preserved
    }
    const std::vector<uint32_t> sorted(job->sorted, job->sorted + job->n_sorted);
    // the layout (part_walk.hpp): offsets, slots per bucket, the heavy list, one task per slot
    std::vector<PartTask> tasks;
    uint32_t nheavy = 0;
    job->offsets[0] = 0;
    job->task_off[0] = 0;
    memset(job->heavy, 0, ((size_t)M + 1) * sizeof(uint32_t));
    for (uint32_t b = 0; b < M; ++b) {
        const uint32_t off = job->offsets[b], n = job->counts[b], np = part_count(n, (uint32_t)lmax);
        job->offsets[b + 1] = off + n;
        job->task_off[b + 1] = job->task_off[b] + np;
        if (np > HEAVY_PARTS) job->heavy[1 + nheavy++] = b;
        if (!np) continue;
        const uint32_t q = n / np, r = n - q * np;
        for (uint32_t p = 0; p < np; ++p) {
            const uint32_t l0 = part_long_before(p, r, np), l1 = part_long_before(p + 1, r, np);
            tasks.push_back(PartTask{off + p * q + l0, q + (l1 - l0), job->task_off[b] + p});
        }
    }
    job->heavy[0] = nheavy;
    if (tasks.size() > job->record_cap) return G16_ERR_INTERNAL;
    job->n_records = tasks.size();
    std::vector<Raw> records(tasks.size());
    for (const PartTask& t : tasks) {
        AccParked<F30, ParkedArrayStore<F30>> acc;
        acc.inf = true;
        walk_bucket_part<F30>(t, t.len, sorted.data(), table.data(), job->shift, job->base_count, merged != 0, acc, &records[t.slot]);
    }
    if (!records.empty()) memcpy(job->records, records.data(), records.size() * sizeof(Raw));
    // the fold on the exact host group law: sum_w 2^(c w) sum_b (b + 1) S_(w,b) (per-window) or sum_k (k + 1) S_k (merged)
    std::vector<X> sums(M, X::identity());
    for (uint32_t b = 0; b < M; ++b)
        for (uint32_t s = job->task_off[b]; s < job->task_off[b + 1]; ++s) sums[b].add(Acc30<F30>::load_raw(records[s]).to_std());
    auto weighted = [&](uint32_t lo, uint32_t hi) {   // sum_{lo <= b < hi} (b - lo + 1) S_b by running sums from the top
        X run = X::identity(), tot = X::identity();
        for (uint32_t b = hi; b-- > lo;) { run.add(sums[b]); tot.add(run); }
        return tot;
    };
    X res = X::identity();
    if (merged) res = weighted(0, M);
    else
        for (int w = groups; w-- > 0;) {
            for (int k = 0; k < c; ++k) res = res.dbl();
            res.add(weighted((uint32_t)w * B, (uint32_t)(w + 1) * B));
        }
    const A out = res.to_affine();
    memcpy(job->out_affine, &out, sizeof(A));
    return G16_OK;
}

}  // namespace

extern "C" int g16_host_msm_parts_lab(int curve, int merged, int c, int groups, int lmax, int rows, g16_pass_lab_job* job) {
    if (curve == G16_BLS12_381) return parts_lab_host<Bls12_381>(merged, c, groups, lmax, rows, job);
    if (curve == G16_BN254) return parts_lab_host<Bn254>(merged, c, groups, lmax, rows, job);
    return G16_ERR_BAD_ARG;
}
