// Unit-level entry points behind the C ABI: witness map, distributed-map stages, ad-hoc MSMs, a single NTT, and the CPU-side
// self-test hooks (field / group operations, the bucket-method model).
#pragma once
#include "api_types.hpp"
#include "prover.hpp"
#include "part_walk.hpp"

namespace {

template <class C>
struct UnitApi {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef typename C::G1A G1A;
    typedef typename C::G2A G2A;
    typedef typename C::G1X G1X;
    typedef typename C::G2X G2X;
    static constexpr int L = Fq::N / 2;  // 64-bit limbs per Fq
    // ---------------------------------------------------------------------------------------
    static int witness_map_api(g16_ctx* ctx, const g16_circuit* ckh, const uint64_t* z, uint64_t n_assign, int on_device, uint64_t* h_out) {
        const DeviceCircuit<C>* ck = static_cast<const DeviceCircuit<C>*>(ckh->dc);
        if (n_assign != ck->num_variables) return G16_ERR_BAD_LENGTH;
        DrainOnError drain(ctx);
        ctx->reset_arena();
        const Fr* d_z = nullptr;
        G16_TRY(Prover<C>::stage_assignment(ctx, z, n_assign, on_device, &d_z));
        Fr* d_h = nullptr;
        G16_TRY(ctx->arena.alloc_n(ck->dom->n, &d_h));
        // the map alone between two events (g16_timings.witness_map_ms / ntt_ms, as g16_prove records them): neither the staging of a
        // host assignment before it nor the download of h after it
        ctx->t_ntt[0].used = ctx->t_ntt[1].used = false;
        G16_TRY(ctx->t_wm.start(ctx->stream));
        G16_TRY((witness_map_device<C>(ck, d_z, d_h, ctx->arena, ctx->stream, ctx->t_ntt)));
        G16_TRY(ctx->t_wm.stop(ctx->stream));
        G16_HIP_TRY(hipMemcpyAsync(h_out, d_h, ck->dom->n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        G16_HIP_TRY(hipStreamSynchronize(ctx->stream));
        drain.dismiss();
        ctx->tm.witness_map_ms = ctx->t_wm.ms();
        ctx->tm.ntt_ms = ctx->t_ntt[0].ms() + ctx->t_ntt[1].ms();
        return G16_OK;
    }

    // async: enqueue on the witness-map stream and return (the caller's exchange goes on that stream too: g16_ctx_wm_stream)
    static int dwm_stage_api(g16_ctx* ctx, const g16_circuit* ckh, const void* dwp, int stage, const uint64_t* z, uint64_t n_assign, int on_device,
                             uint64_t* const work[3], uint64_t* const recv[3], uint64_t* h_local, bool async) {
        const DeviceCircuit<C>* ck = static_cast<const DeviceCircuit<C>*>(ckh->dc);
        const DistWm<C>* dw = static_cast<const DistWm<C>*>(dwp);
        DrainOnError drain(ctx);
        const Fr* d_z = nullptr;
        if (stage == 0) {
            if (!z || n_assign != ck->num_variables) return G16_ERR_BAD_LENGTH;
            if (async) {
                if (!on_device) return G16_ERR_BAD_ARG;   // a staged host copy would live in the arena the next call resets
                d_z = reinterpret_cast<const Fr*>(z);
            } else {
                ctx->reset_arena();
                G16_TRY(Prover<C>::stage_assignment(ctx, z, n_assign, on_device, &d_z));
            }
        }
        Fr* w[3] = {reinterpret_cast<Fr*>(work[0]), reinterpret_cast<Fr*>(work[1]), reinterpret_cast<Fr*>(work[2])};
        Fr* rv[3] = {reinterpret_cast<Fr*>(recv[0]), reinterpret_cast<Fr*>(recv[1]), reinterpret_cast<Fr*>(recv[2])};
        G16_TRY((dwm_stage<C>(ck, dw, stage, d_z, w, rv, reinterpret_cast<Fr*>(h_local), async ? ctx->stream_wm : ctx->stream)));
        if (!async) G16_HIP_TRY(hipStreamSynchronize(ctx->stream));   // the caller's exchange runs on its own stream
        drain.dismiss();
        return G16_OK;
    }

    // shard_n > 1: rank shard_r's bucket-space share of the MSM (window tables built on the fly, merged windows): the ranks' results
    // add up to the MSM
    template <class F>
    static int msm_api(g16_ctx* ctx, const uint64_t* bases, const uint64_t* scalars, uint64_t n, uint64_t* out_affine, int shard_n = 1,
                       int shard_r = 0) {
        typedef Affine<F> A;
        typedef XYZZ<F> X;
        hipStream_t st = ctx->stream;
        DrainOnError drain(ctx);
        ctx->reset_arena();
        A* d_b = nullptr;
        Fr* d_s = nullptr;
        G16_TRY(ctx->arena.alloc_n(n ? n : 1, &d_b));
        G16_TRY(ctx->arena.alloc_n(n ? n : 1, &d_s));
        if (n) {
            G16_HIP_TRY(hipMemcpyAsync(d_b, bases, n * sizeof(A), hipMemcpyHostToDevice, st));
            G16_HIP_TRY(hipMemcpyAsync(d_s, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, st));
        }
        // ad-hoc bases: per-window buckets.  G16_MSM_API_PRECOMP=1 routes this entry point through the proving-key path
        // instead (window tables built on the fly, merged windows) so that it can be tested on arbitrary inputs.
        int merged_c = 0;
        const char* e = getenv("G16_MSM_API_PRECOMP");
        uint32_t modw[Fr::N];
        for (int i = 0; i < Fr::N; ++i) modw[i] = Fr::Params::mod(i);
        if (((e && atoi(e) != 0) || shard_n > 1) && n) merged_c = merged_window_bits(n, Fr::Params::BITS, modw, Fr::N);
        if (shard_n > 1 && n && !merged_c) return G16_ERR_BAD_ARG;   // G16_MSM_PRECOMP=0 / too many points for merged entries
        if (shard_n > 1 && !n) { memset(out_affine, 0, sizeof(A)); drain.dismiss(); return G16_OK; }
        if (merged_c) {
            const int W = msm_plan_windows(merged_c, Fr::Params::BITS, modw, Fr::N);
            A* d_t = nullptr;
            G16_TRY(ctx->arena.alloc_n((size_t)n * W, &d_t));
            G16_TRY((build_window_tables<F>(d_b, n, merged_c, W, d_t, st)));
            d_b = d_t;
        } else {
            G16_TRY((convert_bases<F>(d_b, n, st)));
        }
        ScalarSort ss;
        G16_TRY((sort_scalars<C>(d_s, n, merged_c, ctx->arena, st, &ss, shard_n, shard_r)));
        MsmBuffers<F> buf;
        G16_TRY((msm_bucket_pass<F>(d_b, 0, n, ss, ctx->arena, st, &buf, &ctx->t_bucket[0])));
        G16_TRY((msm_reduce<F>(buf, ss, st)));
        std::vector<X> hws(ss.plan.outputs());
        G16_HIP_TRY(hipMemcpyAsync(hws.data(), buf.window_sums, sizeof(X) * ss.plan.outputs(), hipMemcpyDeviceToHost, st));
        G16_HIP_TRY(hipStreamSynchronize(st));
        drain.dismiss();
        const A res = fold_windows<F>(hws.data(), ss.plan).to_affine();
        memcpy(out_affine, &res, sizeof(A));
        ctx->tm.bucket_pass_ms = ctx->t_bucket[0].ms();
        ctx->tm.bucket_ms[0] = ctx->tm.bucket_pass_ms;
        ctx->tm.window_bits = ss.plan.c;
        ctx->tm.windows = ss.plan.W;
        return G16_OK;
    }

    // The reductions alone on caller-made partial sums (test hooks, g16_dev_msm_reduce_lab and g16_dev_msm_reduce_batch_lab): a plan, and
    // per job a ScalarSort -- slot offsets and the heavy list by bucket_slots_kernel's rule for a segment length of 1: one partial per
    // entry, more than HEAVY_PARTS is heavy -- and the buffers are filled here; the kernels are launched by msm_reduce / msm_reduce_batch /
    // msm_heavy_reduce[_batch] and the sums folded by fold_windows, as in a proof.
    template <class F>
    struct ReduceLabJob {
        typedef Fp30<typename Fq::Params> B30;
        typedef AccRaw<typename std::conditional<std::is_same<F, Fq>::value, B30, Fp2x30<typename Fq::Params>>::type> Raw;
        static constexpr size_t REC_WORDS = (std::is_same<F, Fq>::value ? 4 : 8) * B30::NL;
        static_assert(sizeof(Raw) == REC_WORDS * sizeof(uint32_t), "a record is its limbs, nothing else");
        ScalarSort ss;
        MsmBuffers<F> buf;
        uint64_t n_records = 0;
        std::vector<uint32_t> task_off, heavy, after;
        std::vector<XYZZ<F>> hws;
    };
    static int reduce_lab_plan(int merged, int c, int groups, int G, MsmPlan* plan) {
        if (c < 2 || c > 16 || groups < 1 || groups > 32 || (G != 8 && G != 16 && G != 32)) return G16_ERR_BAD_ARG;
        plan->c = c;
        plan->W = groups;
        plan->groups = groups;
        plan->merged = merged != 0;
        plan->B = 1u << (c - 1);
        plan->G = (uint32_t)G;
        plan->Lmax = 1;
        plan->chunk = 1024;
        for (int k = 0; k < 10; ++k) plan->K[k] = 0;
        if (plan->outputs() > MSM_MAX_OUTPUTS) return G16_ERR_BAD_ARG;
        return G16_OK;
    }
    // host half of a job: slot offsets and the heavy list from nparts (nothing on the device yet)
    template <class F>
    static int reduce_lab_layout(const MsmPlan& plan, const uint32_t* nparts, uint64_t n_records, ReduceLabJob<F>* job) {
        const uint32_t M = plan.buckets();
        job->ss.plan = plan;
        job->n_records = n_records;
        job->task_off.assign((size_t)M + 1, 0u);
        job->heavy.assign((size_t)M + 1, 0u);
        uint64_t total = 0;
        for (uint32_t b = 0; b < M; ++b) {
            job->task_off[b] = (uint32_t)total;
            total += nparts[b];
            if (nparts[b] > HEAVY_PARTS) job->heavy[1 + job->heavy[0]++] = b;
            if (total >= ((uint64_t)1 << 31)) return G16_ERR_BAD_LENGTH;
        }
        job->task_off[M] = (uint32_t)total;
        if (total != n_records) return G16_ERR_BAD_LENGTH;
        job->ss.max_tasks = (uint32_t)total;
        return G16_OK;
    }
    // device half: the job's own buffers from the arena, layout and records uploaded
    template <class F>
    static int reduce_lab_upload(g16_ctx* ctx, const uint32_t* records, ReduceLabJob<F>* job) {
        typedef typename ReduceLabJob<F>::Raw Raw;
        const MsmPlan& plan = job->ss.plan;
        const uint32_t M = plan.buckets();
        const uint64_t n_records = job->n_records;
        hipStream_t st = ctx->stream;
        Raw *d_partials = nullptr, *d_chunk = nullptr;
        G16_TRY(ctx->arena.alloc_n((size_t)M + 1, &job->ss.task_off));
        G16_TRY(ctx->arena.alloc_n((size_t)M + 1, &job->ss.heavy));
        G16_TRY(ctx->arena.alloc_n(n_records ? (size_t)n_records : 1, &d_partials));
        G16_TRY(ctx->arena.alloc_n((size_t)plan.chunks() * plan.groups * 2, &d_chunk));
        G16_TRY(ctx->arena.alloc_n((size_t)plan.outputs(), &job->buf.window_sums));
        job->buf.partials = d_partials;
        job->buf.chunk_out = d_chunk;
        G16_HIP_TRY(hipMemcpyAsync(job->ss.task_off, job->task_off.data(), ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        G16_HIP_TRY(hipMemcpyAsync(job->ss.heavy, job->heavy.data(), ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (n_records) G16_HIP_TRY(hipMemcpyAsync(d_partials, records, (size_t)n_records * sizeof(Raw), hipMemcpyHostToDevice, st));
        return G16_OK;
    }
    // the group sums and the records as the reductions left them, enqueued behind the kernels
    template <class F>
    static int reduce_lab_download(g16_ctx* ctx, ReduceLabJob<F>* job) {
        typedef typename ReduceLabJob<F>::Raw Raw;
        const MsmPlan& plan = job->ss.plan;
        hipStream_t st = ctx->stream;
        job->hws.resize(plan.outputs());
        job->after.resize((size_t)job->n_records * ReduceLabJob<F>::REC_WORDS);
        G16_HIP_TRY(hipMemcpyAsync(job->hws.data(), job->buf.window_sums, sizeof(XYZZ<F>) * plan.outputs(), hipMemcpyDeviceToHost, st));
        if (job->n_records)
            G16_HIP_TRY(hipMemcpyAsync(job->after.data(), job->buf.partials, (size_t)job->n_records * sizeof(Raw), hipMemcpyDeviceToHost, st));
        return G16_OK;
    }
    // after the stream has drained: every bucket's first slot, and the fold
    template <class F>
    static void reduce_lab_finish(const ReduceLabJob<F>& job, const uint32_t* nparts, uint32_t* first_slots, uint64_t* out_affine) {
        typedef typename ReduceLabJob<F>::Raw Raw;
        constexpr size_t REC_WORDS = ReduceLabJob<F>::REC_WORDS;
        const MsmPlan& plan = job.ss.plan;
        const uint32_t M = plan.buckets();
        for (uint32_t b = 0; b < M; ++b) {
            uint32_t* o = first_slots + (size_t)b * REC_WORDS;
            if (nparts[b]) memcpy(o, job.after.data() + (size_t)job.task_off[b] * REC_WORDS, sizeof(Raw));
            else memset(o, 0, sizeof(Raw));
        }
        const Affine<F> res = fold_windows<F>(job.hws.data(), plan).to_affine();
        memcpy(out_affine, &res, sizeof(Affine<F>));
    }

    template <class F>
    static int msm_reduce_lab(g16_ctx* ctx, int merged, int c, int groups, int G, const uint32_t* nparts, const uint32_t* records,
                              uint64_t n_records, uint32_t* first_slots, uint64_t* out_affine) {
        MsmPlan plan;
        G16_TRY(reduce_lab_plan(merged, c, groups, G, &plan));
        ReduceLabJob<F> job;
        G16_TRY(reduce_lab_layout<F>(plan, nparts, n_records, &job));
        hipStream_t st = ctx->stream;
        DrainOnError drain(ctx);
        ctx->reset_arena();
        G16_TRY(reduce_lab_upload<F>(ctx, records, &job));
        G16_TRY((msm_reduce<F>(job.buf, job.ss, st)));
        G16_TRY(reduce_lab_download<F>(ctx, &job));
        G16_HIP_TRY(hipStreamSynchronize(st));
        drain.dismiss();
        reduce_lab_finish<F>(job, nparts, first_slots, out_affine);
        return G16_OK;
    }

    // The batch form (g16_dev_msm_reduce_batch_lab; G1: the prover batches no G2 reductions and msm_reduce_batch is built for Fq alone):
    // 1 to REDUCE_LAB_JOBS jobs over one plan, each with its own slot offsets, heavy list and buffers, reduced by the launches
    // prove_partial makes.  mode 0 ("together"): msm_reduce_batch(all, heavy_done = false), the last batch with h inside.  mode 1
    // ("early"): the jobs of early_mask go through msm_heavy_reduce_batch as one launch, every other job through msm_heavy_reduce
    // alone, then msm_reduce_batch(all, heavy_done = true): the single-GPU proof, whose first batch has its first stage underneath the h
    // pass.  Refused (G16_ERR_BAD_ARG): n_jobs outside 1 .. 4, an unknown mode, in early mode a subset that is empty or names a job that
    // is not there.
    static constexpr int REDUCE_LAB_JOBS = 4;
    static int msm_reduce_batch_lab(g16_ctx* ctx, int merged, int c, int groups, int G, int n_jobs, int mode, uint32_t early_mask,
                                    const uint32_t* const* nparts, const uint32_t* const* records, const uint64_t* n_records,
                                    uint32_t* const* first_slots, uint64_t* const* out_affine) {
        typedef Fq F;
        if (n_jobs < 1 || n_jobs > REDUCE_LAB_JOBS || (mode != 0 && mode != 1)) return G16_ERR_BAD_ARG;
        if (mode == 1 && (early_mask == 0 || (early_mask >> n_jobs) != 0)) return G16_ERR_BAD_ARG;
        for (int j = 0; j < n_jobs; ++j)
            if (!nparts[j] || !first_slots[j] || !out_affine[j] || (n_records[j] && !records[j])) return G16_ERR_BAD_ARG;
        MsmPlan plan;
        G16_TRY(reduce_lab_plan(merged, c, groups, G, &plan));
        ReduceLabJob<F> jobs[REDUCE_LAB_JOBS];
        for (int j = 0; j < n_jobs; ++j) G16_TRY(reduce_lab_layout<F>(plan, nparts[j], n_records[j], &jobs[j]));
        hipStream_t st = ctx->stream;
        DrainOnError drain(ctx);
        ctx->reset_arena();
        const MsmBuffers<F>* bufs[REDUCE_LAB_JOBS];
        const ScalarSort* sorts[REDUCE_LAB_JOBS];
        for (int j = 0; j < n_jobs; ++j) {
            G16_TRY(reduce_lab_upload<F>(ctx, records[j], &jobs[j]));
            bufs[j] = &jobs[j].buf;
            sorts[j] = &jobs[j].ss;
        }
        if (mode == 1) {
            const MsmBuffers<F>* eb[REDUCE_LAB_JOBS];
            const ScalarSort* es[REDUCE_LAB_JOBS];
            int ne = 0;
            for (int j = 0; j < n_jobs; ++j)
                if ((early_mask >> j) & 1u) { eb[ne] = bufs[j]; es[ne] = sorts[j]; ++ne; }
            G16_TRY((msm_heavy_reduce_batch<F>(eb, es, ne, st)));
            for (int j = 0; j < n_jobs; ++j)
                if (!((early_mask >> j) & 1u)) G16_TRY((msm_heavy_reduce<F>(*bufs[j], *sorts[j], st)));
        }
        G16_TRY((msm_reduce_batch<F>(bufs, sorts, n_jobs, st, /*heavy_done=*/mode == 1)));
        for (int j = 0; j < n_jobs; ++j) G16_TRY(reduce_lab_download<F>(ctx, &jobs[j]));
        G16_HIP_TRY(hipStreamSynchronize(st));
        drain.dismiss();
        for (int j = 0; j < n_jobs; ++j) reduce_lab_finish<F>(jobs[j], nparts[j], first_slots[j], out_affine[j]);
        return G16_OK;
    }

    // The bucket pass's walk in place (test hook, g16_dev_msm_pass_lab): a plan filled by hand as above; per job a table, a bucket
    // histogram and a sorted list the caller made.  offsets, task_off and the heavy list come from msm_slot_layout (the tail of
    // sort_scalars), the passes of all jobs go as ONE launch of msm_bucket_pass_batch, then msm_reduce and fold_windows per job.
    // msm_bucket_pass_batch allocates the partial-sum slots itself, from the arena and unzeroed.  The lab makes the same allocations
    // first, fills them with 0xA5, and rewinds the arena, so that the batch call's own allocations land on the filled memory; that they
    // did is checked afterwards (G16_ERR_INTERNAL).  ss.max_tasks = task_off[M] + 8: the 8 records behind the last slot are the guards.
    // Refused (G16_ERR_BAD_ARG): whatever would let the kernel read outside what was uploaded.  A point index outside [0, base_count)
    // after `shift` is NOT refused: skipping it is the kernel's to do.
    // parts (g16_dev_msm_parts_lab): the same with the bucket-part walk -- plan.walk = MSM_WALK_PARTS, lseg is the longest part, the
    // layout and the task list come from msm_parts_layout, a bucket's slots are its parts; per-window plans run it here too.
    template <class F>
    static int msm_pass_lab(g16_ctx* ctx, int merged, int c, int groups, int G, int lseg, int rows, g16_pass_lab_job* jobs, int n_jobs,
                            bool parts = false) {
        typedef Affine<F> A;
        typedef XYZZ<F> X;
        typedef Fp30<typename Fq::Params> B30;
        typedef AccRaw<typename std::conditional<std::is_same<F, Fq>::value, B30, Fp2x30<typename Fq::Params>>::type> Raw;
        constexpr size_t REC_WORDS = (std::is_same<F, Fq>::value ? 4 : 8) * B30::NL;
        constexpr uint32_t GUARDS = 8;
        constexpr int MAX_JOBS = 4;
        if (n_jobs < 1 || n_jobs > MAX_JOBS || !jobs) return G16_ERR_BAD_ARG;
        if (c < 2 || c > 16 || groups < 1 || groups > 32 || (G != 8 && G != 16 && G != 32) || lseg < 8 || lseg > 4096) return G16_ERR_BAD_ARG;
        if (rows < 1 || rows > 32 || (!merged && rows != 1)) return G16_ERR_BAD_ARG;
        ScalarSort ss[MAX_JOBS];
        for (int j = 0; j < n_jobs; ++j) {
            MsmPlan& plan = ss[j].plan;
            plan.c = c;
            plan.W = groups;
            plan.groups = groups;
            plan.merged = merged != 0;
            plan.B = 1u << (c - 1);
            plan.G = (uint32_t)G;
            plan.Lmax = (uint32_t)lseg;
            plan.walk = parts ? MSM_WALK_PARTS : MSM_WALK_SEGMENT;
            plan.chunk = 1024;
            for (int k = 0; k < 10; ++k) plan.K[k] = 0;
        }
        const MsmPlan& plan = ss[0].plan;
        if (plan.outputs() > MSM_MAX_OUTPUTS) return G16_ERR_BAD_ARG;
        const uint32_t M = plan.buckets();
        if (M > (1u << 12)) return G16_ERR_BAD_ARG;
        for (int j = 0; j < n_jobs; ++j) {
            const g16_pass_lab_job& job = jobs[j];
            if (!job.counts || !job.records || !job.offsets || !job.task_off || !job.heavy || !job.out_affine) return G16_ERR_BAD_ARG;
            if (job.n_sorted > ((uint64_t)1 << 16) || (job.n_sorted && !job.sorted)) return G16_ERR_BAD_ARG;
            if (job.base_count > ((uint64_t)1 << 16) || (job.base_count && !job.table)) return G16_ERR_BAD_ARG;
            if (job.shift > ((int64_t)1 << 40) || job.shift < -((int64_t)1 << 40)) return G16_ERR_BAD_ARG;
            uint64_t total = 0;
            for (uint32_t b = 0; b < M; ++b) total += job.counts[b];
            if (total != job.n_sorted) return G16_ERR_BAD_ARG;
            if (merged)
                for (uint64_t e = 0; e < job.n_sorted; ++e)
                    if (((job.sorted[e] >> 26) & 31u) >= (uint32_t)rows) return G16_ERR_BAD_ARG;
            // a bucket gets one slot per segment it touches: <= segments + buckets in total; one per part: <= entries / lseg + buckets
            const uint64_t slots = (parts ? job.n_sorted / (uint64_t)lseg : (job.n_sorted + (uint64_t)lseg - 1) / (uint64_t)lseg) + M;
            if (job.record_cap < slots + GUARDS) return G16_ERR_BAD_LENGTH;
        }
        hipStream_t st = ctx->stream;
        DrainOnError drain(ctx);
        ctx->reset_arena();
        A* d_table[MAX_JOBS] = {};
        uint32_t *d_counts[MAX_JOBS] = {}, *d_nparts = nullptr, *d_block = nullptr;
        std::vector<uint32_t> h_task((size_t)MAX_JOBS * (M + 1));
        for (int j = 0; j < n_jobs; ++j) {
            const g16_pass_lab_job& job = jobs[j];
            const size_t npts = (size_t)rows * job.base_count;
            G16_TRY(ctx->arena.alloc_n(npts ? npts : 1, &d_table[j]));
            G16_TRY(ctx->arena.alloc_n((size_t)M, &d_counts[j]));
            G16_TRY(ctx->arena.alloc_n(job.n_sorted ? (size_t)job.n_sorted : 1, &ss[j].sorted));
            G16_TRY(ctx->arena.alloc_n((size_t)M + 1, &ss[j].offsets));
            G16_TRY(ctx->arena.alloc_n((size_t)M + 1, &ss[j].task_off));
            G16_TRY(ctx->arena.alloc_n((size_t)M + 1, &ss[j].heavy));
            if (!d_nparts) {
                G16_TRY(ctx->arena.alloc_n((size_t)M, &d_nparts));
                G16_TRY(ctx->arena.alloc_n((size_t)M / 2048 + 1, &d_block));
            }
            if (npts) {
                G16_HIP_TRY(hipMemcpyAsync(d_table[j], job.table, npts * sizeof(A), hipMemcpyHostToDevice, st));
                G16_TRY((convert_bases<F>(d_table[j], npts, st)));
            }
            G16_HIP_TRY(hipMemcpyAsync(d_counts[j], job.counts, (size_t)M * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            if (job.n_sorted)
                G16_HIP_TRY(hipMemcpyAsync(ss[j].sorted, job.sorted, (size_t)job.n_sorted * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            G16_HIP_TRY(hipMemsetAsync(ss[j].heavy, 0, ((size_t)M + 1) * sizeof(uint32_t), st));
            if (parts) {
                G16_TRY(ctx->arena.alloc_n((size_t)(job.n_sorted / (uint64_t)lseg) + M, &ss[j].tasks));
                uint32_t* scratch = nullptr;
                G16_TRY(ctx->arena.alloc_n(msm_parts_layout_scratch(M, plan.Lmax), &scratch));
                G16_TRY(msm_parts_layout(d_counts[j], M, plan.Lmax, ss[j].offsets, d_nparts, ss[j].task_off, ss[j].heavy, ss[j].tasks, scratch, st));
            } else
                G16_TRY(msm_slot_layout(d_counts[j], M, 0, plan.Lmax, ss[j].offsets, d_nparts, ss[j].task_off, ss[j].heavy, d_block, st));
            G16_HIP_TRY(hipMemcpyAsync(h_task.data() + (size_t)j * (M + 1), ss[j].task_off, ((size_t)M + 1) * sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, st));
        }
        G16_HIP_TRY(hipStreamSynchronize(st));
        for (int j = 0; j < n_jobs; ++j) {
            const uint32_t tasks = h_task[(size_t)j * (M + 1) + M];
            if ((uint64_t)tasks + GUARDS > jobs[j].record_cap) return G16_ERR_INTERNAL;   // more slots than segments + buckets
            ss[j].n = jobs[j].n_sorted;
            ss[j].max_sorted = jobs[j].n_sorted;
            ss[j].max_tasks = tasks + GUARDS;
            // one task past the last segment: real plans size the grid by an upper bound too, and that task must return at once
            // (parts: one task past the last descriptor)
            if (parts) ss[j].max_segments = jobs[j].n_sorted ? tasks + 1u : 0u;
            else ss[j].max_segments = jobs[j].n_sorted ? (uint32_t)((jobs[j].n_sorted + plan.Lmax - 1) / plan.Lmax) + 1u : 0u;
            jobs[j].n_records = tasks;
        }
        // the allocations msm_bucket_pass_batch is about to make (alloc_msm_buffers, job by job), filled, then handed back
        std::vector<size_t> used;
        for (const Arena::Chunk& ch : ctx->arena.chunks) used.push_back(ch.used);
        Raw* expect[MAX_JOBS] = {};
        for (int j = 0; j < n_jobs; ++j) {
            Raw* chunk_out = nullptr;
            X* sums = nullptr;
            G16_TRY(ctx->arena.alloc_n((size_t)ss[j].max_tasks, &expect[j]));
            G16_TRY(ctx->arena.alloc_n((size_t)plan.chunks() * plan.groups * 2, &chunk_out));
            G16_TRY(ctx->arena.alloc_n((size_t)plan.outputs(), &sums));
            G16_HIP_TRY(hipMemsetAsync(expect[j], 0xA5, (size_t)ss[j].max_tasks * sizeof(Raw), st));
        }
        for (size_t k = 0; k < ctx->arena.chunks.size(); ++k) ctx->arena.chunks[k].used = k < used.size() ? used[k] : 0;
        MsmBuffers<F> buf[MAX_JOBS];
        PassJob<F> pj[MAX_JOBS];
        for (int j = 0; j < n_jobs; ++j) pj[j] = PassJob<F>{d_table[j], jobs[j].shift, jobs[j].base_count, &ss[j], &buf[j]};
        G16_TRY((msm_bucket_pass_batch<F>(pj, n_jobs, ctx->arena, st, nullptr)));
        for (int j = 0; j < n_jobs; ++j)
            if (buf[j].partials != (void*)expect[j]) return G16_ERR_INTERNAL;
        // the records as the pass left them, before the reductions combine them in place
        for (int j = 0; j < n_jobs; ++j) {
            G16_HIP_TRY(hipMemcpyAsync(jobs[j].records, buf[j].partials, (size_t)ss[j].max_tasks * sizeof(Raw), hipMemcpyDeviceToHost, st));
            G16_HIP_TRY(hipMemcpyAsync(jobs[j].offsets, ss[j].offsets, ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            G16_HIP_TRY(hipMemcpyAsync(jobs[j].heavy, ss[j].heavy, ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            memcpy(jobs[j].task_off, h_task.data() + (size_t)j * (M + 1), ((size_t)M + 1) * sizeof(uint32_t));
        }
        std::vector<X> hws((size_t)MAX_JOBS * plan.outputs());
        for (int j = 0; j < n_jobs; ++j) {
            G16_TRY((msm_reduce<F>(buf[j], ss[j], st)));
            G16_HIP_TRY(hipMemcpyAsync(hws.data() + (size_t)j * plan.outputs(), buf[j].window_sums, sizeof(X) * plan.outputs(),
                                       hipMemcpyDeviceToHost, st));
        }
        G16_HIP_TRY(hipStreamSynchronize(st));
        drain.dismiss();
        for (int j = 0; j < n_jobs; ++j) {
            const A res = fold_windows<F>(hws.data() + (size_t)j * plan.outputs(), plan).to_affine();
            memcpy(jobs[j].out_affine, &res, sizeof(A));
        }
        return G16_OK;
    }

    // Digits and sort layout in place (test hook, g16_dev_msm_sort_lab): the scalars go up, sort_scalars runs as msm_api and the prover
    // call it (the environment knobs apply), and the plan, the layout and the sorted list come back.
    static int msm_sort_lab(g16_ctx* ctx, const uint64_t* scalars, uint64_t n, int merged_c, int shard_n, int shard_r, g16_sort_lab_info* info,
                            uint32_t* offsets, uint32_t* task_off, uint32_t* heavy, uint64_t bucket_cap, uint32_t* sorted, uint64_t sorted_cap) {
        if (n > ((uint64_t)1 << 16) || shard_n < 1 || shard_n > 64 || shard_r < 0 || shard_r >= shard_n || (shard_n > 1 && merged_c <= 0))
            return G16_ERR_BAD_ARG;
        if (merged_c && (merged_c < MSM_MERGED_MIN_C || merged_c > MSM_MERGED_MAX_C)) return G16_ERR_BAD_ARG;
        hipStream_t st = ctx->stream;
        DrainOnError drain(ctx);
        ctx->reset_arena();
        Fr* d_s = nullptr;
        G16_TRY(ctx->arena.alloc_n(n ? (size_t)n : 1, &d_s));
        if (n) G16_HIP_TRY(hipMemcpyAsync(d_s, scalars, (size_t)n * sizeof(Fr), hipMemcpyHostToDevice, st));
        ScalarSort ss;
        G16_TRY((sort_scalars<C>(d_s, n, merged_c, ctx->arena, st, &ss, shard_n, shard_r)));
        const MsmPlan& plan = ss.plan;
        const uint32_t M = plan.buckets();
        memset(info, 0, sizeof(*info));
        info->c = plan.c; info->W = plan.W; info->groups = plan.groups; info->merged = plan.merged ? 1 : 0;
        info->B = plan.B; info->Lmax = plan.Lmax; info->max_tasks = ss.max_tasks; info->max_segments = ss.max_segments;
        for (int k = 0; k < 10; ++k) info->K[k] = plan.K[k];
        if (plan.affine_levels) return G16_ERR_BAD_ARG;   // padded bucket regions: `sorted` has holes, not this lab's subject
        if ((uint64_t)M + 1 > bucket_cap) return G16_ERR_BAD_LENGTH;
        G16_HIP_TRY(hipMemcpyAsync(offsets, ss.offsets, ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        G16_HIP_TRY(hipMemcpyAsync(task_off, ss.task_off, ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        G16_HIP_TRY(hipMemcpyAsync(heavy, ss.heavy, ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        G16_HIP_TRY(hipStreamSynchronize(st));
        info->n_sorted = offsets[M];
        if ((uint64_t)offsets[M] > ss.max_sorted) return G16_ERR_INTERNAL;   // more entries than the list was allocated for
        if ((uint64_t)offsets[M] > sorted_cap) return G16_ERR_BAD_LENGTH;
        if (offsets[M]) G16_HIP_TRY(hipMemcpy(sorted, ss.sorted, (size_t)offsets[M] * sizeof(uint32_t), hipMemcpyDeviceToHost));
        drain.dismiss();
        return G16_OK;
    }

    // The window-table builder in place (test hook, g16_dev_window_table_lab): the points go up as they are, build_window_tables is
    // called as the key loader and msm_api call it -- it runs its own chunk loop, allocates its own parking buffer and picks its own
    // launch shape; park = nullptr makes it return with the table finished -- and the W * n records come back.  W is NOT checked
    // against the builder's limit here: refusing W = 33 is the builder's to do.
    template <class F>
    static int window_table_lab(g16_ctx* ctx, const uint64_t* points, uint64_t n, int c, int W, uint64_t* table_out) {
        typedef Affine<F> A;
        if (c < 1 || c > 32 || W < 1 || W > 64 || n > ((uint64_t)1 << 18) + 4096) return G16_ERR_BAD_ARG;
        hipStream_t st = ctx->stream;
        DrainOnError drain(ctx);
        ctx->reset_arena();
        A *d_p = nullptr, *d_t = nullptr;
        G16_TRY(ctx->arena.alloc_n(n ? (size_t)n : 1, &d_p));
        G16_TRY(ctx->arena.alloc_n(n ? (size_t)n * W : 1, &d_t));
        if (n) G16_HIP_TRY(hipMemcpyAsync(d_p, points, (size_t)n * sizeof(A), hipMemcpyHostToDevice, st));
        G16_TRY((build_window_tables<F>(d_p, n, c, W, d_t, st)));
        if (n) G16_HIP_TRY(hipMemcpyAsync(table_out, d_t, (size_t)n * W * sizeof(A), hipMemcpyDeviceToHost, st));
        G16_HIP_TRY(hipStreamSynchronize(st));
        drain.dismiss();
        return G16_OK;
    }

    static int ntt_api(g16_ctx* ctx, uint64_t* data, int log_n, int inverse, int coset) {
        if (log_n < 0 || log_n > 30) return G16_ERR_DEGREE_TOO_LARGE;
        hipStream_t st = ctx->stream;
        Domain<C>* dom = nullptr;
        G16_TRY((domain_create<C>(log_n, st, &dom)));
        const size_t n = dom->n;
        ctx->reset_arena();
        Fr *d_a = nullptr, *d_o = nullptr;
        int rc = G16_OK;
        auto body = [&]() -> int {
            G16_TRY(ctx->arena.alloc_n(n, &d_a));
            G16_TRY(ctx->arena.alloc_n(n, &d_o));
            G16_HIP_TRY(hipMemcpyAsync(d_a, data, n * sizeof(Fr), hipMemcpyHostToDevice, st));
            if (!inverse) {
                if (coset) {
                    G16_TRY((domain_ensure_gpow<C>(dom, st)));
                    G16_TRY((scale_by_table<C>(d_a, dom->g_pow, n, st)));
                }
                G16_TRY((ntt_dif<C>(dom, d_a, false, st)));
                G16_TRY((bitrev_scale<C>(dom, d_o, d_a, nullptr, nullptr, st)));
            } else {
                G16_TRY((ntt_dif<C>(dom, d_a, true, st)));
                if (coset) G16_TRY((bitrev_scale<C>(dom, d_o, d_a, dom->s2, nullptr, st)));
                else G16_TRY((bitrev_scale<C>(dom, d_o, d_a, nullptr, &dom->n_inv, st)));
            }
            G16_HIP_TRY(hipMemcpyAsync(data, d_o, n * sizeof(Fr), hipMemcpyDeviceToHost, st));
            G16_HIP_TRY(hipStreamSynchronize(st));
            return G16_OK;
        };
        rc = body();
        domain_destroy<C>(dom);
        return rc;
    }

    // ---------------------------------------------------------------------------------------
    // host-side hooks (no GPU)
    template <class F>
    static int field_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
        F x = load_pod<F>(a), y = b ? load_pod<F>(b) : F::zero(), r;
        switch (op) {
            case 0: r = x + y; break;
            case 1: r = x - y; break;
            case 2: r = x * y; break;
            case 3: r = x.inverse(); break;
            case 4: x.to_canonical(r.v); break;
            case 5: r = F::from_canonical(x.v); break;
            default: return G16_ERR_BAD_ARG;
        }
        memcpy(out, &r, sizeof(F));
        return G16_OK;
    }
    template <class F>
    static int group_op(int op, const uint64_t* p_, const uint64_t* q_, uint64_t* out) {
        typedef Affine<F> A;
        typedef XYZZ<F> X;
        const A p = load_pod<A>(p_);
        X acc = X::from_affine(p);
        if (op == 0) {
            acc.add_affine(load_pod<A>(q_));
        } else if (op == 1) {
            uint32_t k[8];
            memcpy(k, q_, 32);
            acc = acc.mul_bits(k, 256);
        } else if (op == 2) {
            // exercise the projective + projective path with non-trivial ZZ on both sides
            X q = X::from_affine(load_pod<A>(q_));
            X p2 = acc.dbl(), q2 = q.dbl();   // 2p, 2q
            p2.add(q2);                       // 2p + 2q
            X np = acc.neg();
            p2.add(np);                       // p + 2q
            X nq = q.neg();
            p2.add(nq);                       // p + q
            acc = p2;
        } else {
            return G16_ERR_BAD_ARG;
        }
        const A r = acc.to_affine();
        memcpy(out, &r, sizeof(A));
        return G16_OK;
    }
    // CPU model of kernels 1-7 of msm.hip: same plan, same digit/bucket/sign mapping, same chunked running-sum reduction
    // and final fold.  c_override > 0: per-window plan with that window size; < 0: merged plan with window size -c_override
    // (window tables 2^(cj) P_i built here by repeated doubling); 0: per-window plan from the cost model.
    // shard_n > 1 (merged plans): rank shard_r's bucket-space share, exactly as sort_scalars filters and re-indexes the keys
    template <class F>
    static int msm_model(const uint64_t* bases_, const uint64_t* scalars_, uint64_t n, int c_override, uint64_t* out, int shard_n = 1,
                         int shard_r = 0) {
        typedef Affine<F> A;
        typedef XYZZ<F> X;
        uint32_t modw[Fr::N];
        for (int i = 0; i < Fr::N; ++i) modw[i] = Fr::Params::mod(i);
        MsmPlan plan;
        if (c_override > 0) {
            char buf[16];
            snprintf(buf, sizeof(buf), "%d", c_override);
            setenv("G16_MSM_WINDOW", buf, 1);
        }
        if (shard_n > 1 && c_override >= 0) return G16_ERR_BAD_ARG;
        int rc = make_msm_plan(n, Fr::Params::BITS, modw, Fr::N, c_override < 0 ? -c_override : 0, &plan, shard_n, shard_r);
        if (c_override > 0) unsetenv("G16_MSM_WINDOW");
        if (rc) return rc;
        const A* bases = reinterpret_cast<const A*>(bases_);
        std::vector<X> buckets((size_t)plan.buckets(), X::identity());
        for (uint64_t i = 0; i < n; ++i) {
            Fr s;
            memcpy(&s, scalars_ + 4 * i, sizeof(Fr));
            uint32_t can[Fr::N], sp[MSM_SWORDS];
            s.to_canonical(can);
            uint64_t carry = 0;
            for (int k = 0; k < 10; ++k) {
                carry += (uint64_t)(k < Fr::N ? can[k] : 0u) + plan.K[k];
                sp[k] = (uint32_t)carry;
                carry >>= 32;
            }
            sp[10] = 0;
            A p;
            memcpy(&p, bases + i, sizeof(A));
            for (int w = 0; w < plan.W; ++w) {
                if (plan.merged && w) {   // table row w: 2^(c w) P_i
                    X d = X::from_affine(p);
                    for (int k = 0; k < plan.c; ++k) d = d.dbl();
                    p = d.to_affine();
                }
                uint32_t bucket, neg;
                if (!digit_to_bucket(window_raw(sp, w, plan.c), plan.c, &bucket, &neg)) continue;
                if (plan.shard_n > 1) {
                    if (bucket % (uint32_t)plan.shard_n != (uint32_t)plan.shard_r) continue;   // another rank's residue class
                    bucket /= (uint32_t)plan.shard_n;                                            // local index k: b = shard_n k + shard_r
                }
                A q = p;
                if (neg) q.y = q.y.neg();
                // merged: `bucket` is the key over all 2^(c-1) buckets = group * B + bucket-in-group already
                buckets[plan.merged ? (size_t)bucket : (size_t)w * plan.B + bucket].add_affine(q);
            }
        }
        const uint32_t G = plan.chunk_buckets(), cpw = plan.chunks();
        const int NP = plan.planes();
        std::vector<X> wsum(plan.outputs(), X::identity());
        for (int w = 0; w < plan.groups; ++w) {
            for (uint32_t ch = 0; ch < cpw; ++ch) {
                const uint32_t b_lo = ch * G;
                X run = X::identity(), tot = X::identity();
                for (uint32_t bb = G; bb-- > 0;) {
                    run.add(buckets[(size_t)w * plan.B + b_lo + bb]);
                    tot.add(run);
                }
                wsum[(size_t)w * NP + 0].add(tot);                                   // plane 0: weighted chunk sums
                wsum[(size_t)w * NP + 1].add(run);                                   // plane 1: plain chunk sums
                for (int k = 0; k < plan.chunk_bits(); ++k)
                    if ((ch >> k) & 1) wsum[(size_t)w * NP + 2 + k].add(run);        // plane 2 + k: chunks with bit k set
            }
        }
        const A res = fold_windows<F>(wsum.data(), plan).to_affine();
        memcpy(out, &res, sizeof(A));
        return G16_OK;
    }
};

}  // namespace
