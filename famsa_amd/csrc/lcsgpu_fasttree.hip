// lcsgpu_fasttree.hip -- C-ABI entry points for the MedoidTree / PartTree recursion: the leaf matrices
// of a split in one call, the seed assignment of an evaluation, CLARANS (kernels in
// clarans_kernels.hip; here the host side: the two mt19937 streams and the batch of searches).
// The job tables of the batched LCS launches are planned in job_plan.h; staged and launched here.
#include "lcsgpu_internal.h"
#include "fasttree_kernels.h"

#include <functional>
#include <memory>

using namespace lcsgpu_impl;
using lcsgpu::RowsArgs;

static size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// no exception leaves the C-ABI (a std::bad_alloc of the host-side tables would end in std::terminate)
template <class... Params, class... Args>
static int guarded(const char* call, int (*impl)(Params...), Args... args)
{
    try {
        return impl(args...);
    } catch (const std::exception& e) {
        return fail(LCSGPU_E_NOMEM, "%s: %s", call, e.what());
    }
}

// where the tables of every bucket lie in a lane's plan buffers, behind the caller's own table at offset 0
struct PlanLayout {
    struct At { size_t id, end, c0, out, job; };
    std::vector<At> at;
    size_t bytes = 0;
};

// The buckets' tables, behind `head`, into L.h_plan; L.d_plan gets the room.  `reserved` (may be empty): called in between.
static int stage_job_tables(Lane& L, const std::vector<JobBucket>& buckets, const void* head, size_t head_bytes, PlanLayout& lay,
                            const std::function<void()>& reserved = nullptr)
{
    size_t bytes = 0;
    auto take = [&](size_t n) { return std::exchange(bytes, bytes + ((n + 15) & ~(size_t)15)); }; // (16: enough for int64_t and int4)
    take(head_bytes);
    lay.at.clear();
    for (const JobBucket& b : buckets) {
        const size_t nr = b.refs.size();
        lay.at.push_back(PlanLayout::At{take(nr * 4), take(nr * 8), take(nr * 4), take(nr * 8), take(b.jobs.size() * sizeof(Job))});
    }
    lay.bytes = bytes;
    if (L.plan_in_flight) {
        HIP_TRY(hipStreamSynchronize(L.stream));
        L.plan_in_flight = false;
    }
    HIP_TRY(L.h_plan.reserve(L.h_plan.cap ? bytes : bytes * 3 / 2));
    HIP_TRY(L.d_plan.reserve(L.d_plan.cap ? bytes : bytes * 3 / 2));
    if (reserved) reserved();
    char* h = (char*)L.h_plan.p;
    memcpy(h, head, head_bytes);
    for (size_t bi = 0; bi < buckets.size(); ++bi) {
        const JobBucket& b = buckets[bi];
        const PlanLayout::At& at = lay.at[bi];
        for (size_t k = 0; k < b.refs.size(); ++k) {
            ((int32_t*)(h + at.id))[k] = b.refs[k].id;
            ((int64_t*)(h + at.end))[k] = b.refs[k].col_end;
            ((int32_t*)(h + at.c0))[k] = b.refs[k].col0;
            ((int64_t*)(h + at.out))[k] = b.refs[k].out0;
        }
        memcpy(h + at.job, b.jobs.data(), b.jobs.size() * sizeof(Job));
    }
    return LCSGPU_OK;
}

// The staged plan to the device and a launch per bucket into L.d_out, between L.ev_start and L.ev_stop.
static int launch_job_tables(lcsgpu_ctx* ctx, Lane& L, const std::vector<JobBucket>& buckets, const PlanLayout& lay, int mode,
                             const int32_t* d_col_ids, int64_t n_cols, int elem_size)
{
    static_assert(sizeof(Job) == sizeof(int4) && alignof(int4) <= 16, "RowsArgs::jobs");
    RowsArgs a = rows_args_of_set(ctx);
    a.col_ids = d_col_ids;
    a.n_cols = (int32_t)n_cols;
    a.out = L.d_out.p;
    a.elem_size = elem_size;
    a.mode = mode;
    HIP_TRY(hipMemcpyAsync(L.d_plan.p, L.h_plan.p, lay.bytes, hipMemcpyHostToDevice, L.stream));
    L.plan_in_flight = true;
    L.last_launches = 0;
    HIP_TRY(hipEventRecord(L.ev_start, L.stream));
    const char* d = (const char*)L.d_plan.p;
    for (size_t bi = 0; bi < buckets.size(); ++bi) {
        const JobBucket& b = buckets[bi];
        if (b.jobs.empty()) continue;
        const PlanLayout::At& at = lay.at[bi];
        a.n_refs = (int32_t)b.refs.size();
        a.ref_ids = (const int32_t*)(d + at.id);
        a.ref_rows = mode == lcsgpu::MODE_TRIANGLE ? (const int64_t*)(d + at.end) : nullptr;
        a.ref_col0 = (const int32_t*)(d + at.c0);
        a.ref_out0 = (const int64_t*)(d + at.out);
        a.jobs = (const int4*)(d + at.job);
        a.refs_per_block = b.refs_per_wg;
        a.block_threads = b.narrow ? 64 : 0;
        HIP_TRY(lcsgpu::launch_rows(b.bv, b.quirk, a, (int)b.jobs.size(), 1, L.stream));
        trace_lcs_launch(b.bv, b.quirk, a, (long)b.jobs.size());
        ++L.last_launches;
    }
    HIP_TRY(hipEventRecord(L.ev_stop, L.stream));
    L.timing_valid = true;
    return LCSGPU_OK;
}

// The packed LCS triangles of several id lists into lane L's result buffer (device memory), list g at pair offset
// tri_base[g]: validation, planning and the launches of lcsgpu_lcs_triangles_batch.  *count = pairs in total (0: nothing to do).  On return the
// launches are queued on L.stream (or, with a ref beyond 2048 residues in the batch, already finished).
// `before_launch` (may be empty) is called once the plan is made, before the first thing goes to the device: the caller's moment
// to take the compute gate (planning a few hundred lists is tens of milliseconds of host work nobody should wait for).
// square (lcsgpu_dist_text_batch's square form): instead of its triangle every list gets its whole m x m rectangle, row k =
// LCS(ref = member k, partner = every member, itself included), in the kernels' rectangle mode as lcsgpu_assign_seeds_batch
// runs it -- every member is a ref, so the upper half and the diagonal are computed in their own orientation, not mirrored.
static int batch_triangles_to_device(lcsgpu_ctx* ctx, Lane& L, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups,
                                     int elem_size, std::vector<int64_t>& tri_base, int64_t* count_out, bool* had_long,
                                     const std::function<void()>& before_launch = nullptr, bool square = false)
{
    if (!ctx) return fail(LCSGPU_E_INVALID, "NULL ctx");
    if (ctx->n < 0) return fail(LCSGPU_E_STATE, "no sequence set uploaded");
    if (n_groups < 0 || (n_groups > 0 && !group_offsets)) return fail(LCSGPU_E_INVALID, "bad group table");
    if (elem_size != 2 && elem_size != 4) return fail(LCSGPU_E_INVALID, "elem_size must be 2 or 4");
    if (elem_size == 2 && ctx->max_len > 65535)
        return fail(LCSGPU_E_INVALID, "uint16 output needs all sequences <= 65535 residues");
    *count_out = 0;
    *had_long = false;
    if (n_groups == 0) return LCSGPU_OK;
    if (group_offsets[0] != 0) return fail(LCSGPU_E_INVALID, "group_offsets[0] must be 0");
    const int64_t n_total = group_offsets[n_groups];
    if (n_total < 0 || n_total > 0x7fffffff) return fail(LCSGPU_E_INVALID, "bad total id count");
    tri_base.assign((size_t)n_groups + 1, 0);
    bool any_long = false;
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t m = group_offsets[g + 1] - group_offsets[g];
        if (m < 0) return fail(LCSGPU_E_INVALID, "group_offsets not ascending");
        tri_base[g + 1] = tri_base[g] + (square ? m * m : m * (m - 1) / 2);
    }
    const int64_t count = tri_base[n_groups];
    if (count <= 0) return LCSGPU_OK;
    if (!ids) return fail(LCSGPU_E_INVALID, "NULL ids");
    std::vector<uint8_t> cls((size_t)n_total); // lcsgpu_ctx::ref_class of every id: the one pass over the set's tables
    for (int64_t p = 0; p < n_total; ++p) {
        if (ids[p] < 0 || ids[p] >= ctx->n) return fail(LCSGPU_E_INVALID, "id %d out of range", ids[p]);
        cls[(size_t)p] = ctx->ref_class[(size_t)ids[p]];
        any_long |= (cls[(size_t)p] & 0x7f) == 0;
    }
    *count_out = count;
    *had_long = any_long;
    HIP_TRY(hipSetDevice(ctx->device));
    static std::atomic<long> plan_us[4], plan_calls{0}; // LCSGPU_PROFILE
    auto t_mark = std::chrono::steady_clock::now();
    auto lap = [&](int what) {
        const auto t = std::chrono::steady_clock::now();
        plan_us[what] += std::chrono::duration_cast<std::chrono::microseconds>(t - t_mark).count();
        t_mark = t;
    };
    // (a lane that serves these calls serves many of them, of the caller's batch size give or take: one allocation each)
    HIP_TRY(L.d_out.reserve(L.d_out.cap ? (size_t)count * elem_size : (size_t)count * elem_size * 3 / 2));
    lap(0);
    if (any_long) { // the long-ref kernel keeps its 2-D grid: list by list
        if (before_launch) before_launch();
        double ms = 0;
        int launches = 0;
        for (int32_t g = 0; g < n_groups; ++g) {
            const int32_t m = (int32_t)(group_offsets[g + 1] - group_offsets[g]);
            if (m < (square ? 1 : 2)) continue;
            const int32_t* gi = ids + group_offsets[g];
            char* const to = (char*)L.d_out.p + (size_t)tri_base[g] * elem_size;
            int rc = square ? run_rows(ctx, L, lcsgpu::MODE_RECT, gi, 0, m, gi, 0, m, to, m, 0, elem_size)
                            : run_rows(ctx, L, lcsgpu::MODE_TRIANGLE, gi, 0, m, gi, 0, m - 1, to, 0, 0, elem_size);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(L.stream));
            finish_host_call(ctx, L);
            ms += g_last.ms;
            launches += g_last.launches;
        }
        g_last.ms = ms;
        g_last.launches = launches;
        return LCSGPU_OK;
    }

    // the refs: every member but a list's first, which has no partner; rows and columns are positions in `ids`, a ref's
    // columns end at its own row (square: every member, its columns the whole list, its row of the rectangle its own)
    static const int narrow_max = tune_int("narrow_lists", 192); // lists up to that many members run in one-wave workgroups
    double inv_refs[65];
    for (int h = 0; h <= 64; ++h) inv_refs[h] = 1.0 / lcsgpu::refs_per_block_for(h, false, 1, 1);
    std::vector<JobRef> refs;
    refs.reserve((size_t)n_total);
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t g0 = group_offsets[g], g1 = group_offsets[g + 1];
        for (int64_t p = square ? g0 : g0 + 1; p < g1; ++p) {
            const uint8_t c = cls[(size_t)p];
            const bool q = (c & 0x80) != 0;
            const int64_t col_end = square ? g1 : p, out0 = square ? tri_base[g] + (p - g0) * (g1 - g0) : tri_base[g];
            refs.push_back(JobRef{ids[p], g, (int32_t)g0, col_end, out0, q ? 0.0 : (double)((col_end - g0 + 255) / 256) * inv_refs[c], c,
                                  (uint8_t)(q ? lcsgpu::quirk_h_class(ctx->lens[ids[p]]) : 0), !q && g1 - g0 <= narrow_max});
        }
    }
    std::vector<JobBucket> buckets;
    if (!plan_jobs(refs, 1, lcsgpu::refs_per_block_for, buckets)) return fail(LCSGPU_E_INVALID, "batch too large");
    lap(1);
    PlanLayout lay;
    int rc = stage_job_tables(L, buckets, ids, (size_t)n_total * 4, lay, [&] { lap(2); });
    if (rc) return rc;
    lap(3);
    if (getenv("LCSGPU_PROFILE") && (++plan_calls % 20) == 0)
        fprintf(stderr, "triangle batches planned: %ld, thread-ms each: result buffer %.1f, lists + jobs %.1f, plan buffers %.1f, filling them %.1f (last: %lld ids, %d lists)\n",
                plan_calls.load(), 1e-3 * plan_us[0] / plan_calls, 1e-3 * plan_us[1] / plan_calls, 1e-3 * plan_us[2] / plan_calls, 1e-3 * plan_us[3] / plan_calls,
                (long long)n_total, n_groups);
    if (before_launch) before_launch();
    return launch_job_tables(ctx, L, buckets, lay, square ? lcsgpu::MODE_RECT : lcsgpu::MODE_TRIANGLE,
                             (const int32_t*)L.d_plan.p /* its first table */, n_total, elem_size);
}

static int lcs_triangles_batch_impl(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, void* out,
                                    int elem_size)
{
    if (!ctx) return fail(LCSGPU_E_INVALID, "NULL ctx");
    // LCSGPU_PROFILE: where the calls' time goes, summed over the calling threads (printed by the 64th, 128th, ... call)
    static std::atomic<long> prof_us[5], prof_calls{0};
    auto t_mark = std::chrono::steady_clock::now();
    auto lap = [&](int what) {
        const auto t = std::chrono::steady_clock::now();
        prof_us[what] += std::chrono::duration_cast<std::chrono::microseconds>(t - t_mark).count();
        t_mark = t;
    };
    LaneGuard guard(ctx, LaneGuard::ANY);
    Lane& L = guard.lane();
    lap(0);
    std::vector<int64_t> tri_base;
    int64_t count = 0;
    bool had_long = false;
    GateHold hold{ctx->gate}; // from the first launch until the kernels have run
    int rc = batch_triangles_to_device(ctx, L, ids, group_offsets, n_groups, elem_size, tri_base, &count, &had_long, [&] {
        lap(1);
        hold.lock();
        lap(2);
    });
    if (rc || count <= 0) return rc;
    if (!had_long) {
        HIP_TRY(hipEventRecord(L.ev_done, L.stream));
        HIP_TRY(hipEventSynchronize(L.ev_done));
    }
    lap(3);
    hold.release();
    if (!out) return fail(LCSGPU_E_INVALID, "NULL out");
    if (had_long) { // every list was synchronised already; the timing is in g_last
        HIP_TRY(hipMemcpy(out, L.d_out.p, (size_t)count * elem_size, hipMemcpyDeviceToHost));
        return LCSGPU_OK;
    }
    HIP_TRY(hipMemcpyAsync(out, L.d_out.p, (size_t)count * elem_size, hipMemcpyDeviceToHost, L.stream));
    HIP_TRY(hipEventRecord(L.ev_done, L.stream));
    HIP_TRY(hipEventSynchronize(L.ev_done));
    finish_host_call(ctx, L);
    lap(4);
    if (getenv("LCSGPU_PROFILE") && (++prof_calls % 19) == 0)
        fprintf(stderr, "triangles_batch: %ld calls so far, thread-ms per call: lane %.1f, plan %.1f, gate %.1f, kernels %.1f, results to the host %.1f\n",
                prof_calls.load(), 1e-3 * prof_us[0] / prof_calls, 1e-3 * prof_us[1] / prof_calls, 1e-3 * prof_us[2] / prof_calls,
                1e-3 * prof_us[3] / prof_calls, 1e-3 * prof_us[4] / prof_calls);
    return LCSGPU_OK;
}

// What the per-group tree calls (lcsgpu_mst_prim_batch, lcsgpu_upgma_batch) check alike, in the order they always did.
// per_group(g, members) and per_id(id) are the call's own refusals, asked where its limits stood: 0 = go on.
template <class PerGroup, class PerId>
static int check_groups(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, int distance_kind,
                        PerGroup&& per_group, PerId&& per_id)
{
    if (!ctx) return fail(LCSGPU_E_INVALID, "NULL ctx");
    if (ctx->n < 0) return fail(LCSGPU_E_STATE, "no sequence set uploaded");
    if (!valid_kind(distance_kind)) return fail(LCSGPU_E_INVALID, "unknown distance kind %d", distance_kind);
    if (n_groups < 0 || (n_groups > 0 && !group_offsets)) return fail(LCSGPU_E_INVALID, "bad group table");
    if (n_groups == 0) return LCSGPU_OK;
    if (group_offsets[0] != 0) return fail(LCSGPU_E_INVALID, "group_offsets[0] must be 0");
    const int64_t n_total = group_offsets[n_groups];
    if (n_total < 0 || n_total > 0x7fffffff) return fail(LCSGPU_E_INVALID, "bad total id count");
    if (n_total > 0 && !ids) return fail(LCSGPU_E_INVALID, "NULL ids");
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t m = group_offsets[g + 1] - group_offsets[g];
        if (m < 0) return fail(LCSGPU_E_INVALID, "group_offsets not ascending");
        if (int rc = per_group(g, m)) return rc;
    }
    for (int64_t p = 0; p < n_total; ++p) {
        if (ids[p] < 0 || ids[p] >= ctx->n) return fail(LCSGPU_E_INVALID, "id %d out of range", ids[p]);
        if (int rc = per_id(ids[p])) return rc;
    }
    return LCSGPU_OK;
}

// The frame of a per-group tree call: a lane, the lists' 16-bit triangles in its result buffer, the compute gate from
// the first launch until the group kernels have run.
struct GroupCall {
    lcsgpu_ctx* ctx;
    LaneGuard guard;
    Lane& L;
    GateHold hold;
    std::vector<int64_t> tri_base;
    int64_t count = 0;
    bool had_long = false;
    explicit GroupCall(lcsgpu_ctx* c) : ctx(c), guard(c, LaneGuard::ANY), L(guard.lane()), hold{c->gate} {}
    // the launches of lcsgpu_lcs_triangles_batch; then the jobs longest first (the groups that take the most steps start
    // first), each with its triangle's place (Job::tri0 came in as the group)
    template <class GroupJob>
    int triangles(const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, const char* what, std::vector<GroupJob>& jobs)
    {
        int rc = batch_triangles_to_device(ctx, L, ids, group_offsets, n_groups, 2, tri_base, &count, &had_long, [&] { hold.lock(); });
        if (rc) return rc;
        if (count <= 0) return fail(LCSGPU_E_STATE, "the batched %s found no pair to compute", what);
        std::stable_sort(jobs.begin(), jobs.end(), [](const GroupJob& x, const GroupJob& y) { return x.m > y.m; });
        for (GroupJob& job : jobs) job.tri0 = tri_base[(size_t)job.tri0];
        return LCSGPU_OK;
    }
    // once the group kernels are queued (extra_launches of them, on top of the triangles'): the call's kernel time, the
    // wait, the gate; then the caller's copy back and the accounting
    int finish(int extra_launches, const std::function<int()>& copy_back)
    {
        if (!had_long) {
            HIP_TRY(hipEventRecord(L.ev_stop, L.stream));
            L.last_launches += extra_launches;
        }
        HIP_TRY(hipEventRecord(L.ev_done, L.stream));
        HIP_TRY(hipEventSynchronize(L.ev_done));
        hold.release();
        if (int rc = copy_back()) return rc;
        if (!had_long) finish_host_call(ctx, L);
        else L.plan_in_flight = false;
        return LCSGPU_OK;
    }
};

// Prim's MST of many id lists: the lists' triangles by the launches of lcsgpu_lcs_triangles_batch, then ONE launch with a
// workgroup per list (mst_kernels.hip, mst_group_prim_kernel), longest lists first.
static int mst_prim_batch_impl(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, int distance_kind,
                               lcsgpu_mst_edge* out_edges)
{
    const bool triangle_orientation = (distance_kind & LCSGPU_MST_TRIANGLE_ORIENTATION) != 0;
    distance_kind &= ~LCSGPU_MST_TRIANGLE_ORIENTATION;
    // everything that refuses comes first: nothing is computed, out_edges stays as it is
    std::vector<lcsgpu::GroupPrimJob> jobs;
    int64_t n_edges = 0, sq_elems = 0;
    int rc = check_groups(
        ctx, ids, group_offsets, n_groups, distance_kind,
        [&](int32_t g, int64_t m) {
            if (m > LCSGPU_MST_BATCH_MAX_MEMBERS)
                return fail(LCSGPU_E_UNSUPPORTED, "group %d has %lld members: the batched MST handles at most %d (use lcsgpu_mst_prim)", g,
                            (long long)m, LCSGPU_MST_BATCH_MAX_MEMBERS);
            if (m >= 2) {
                jobs.push_back(lcsgpu::GroupPrimJob{(int64_t)g /* the group, until its triangle's place is known */, 0, n_edges, (int32_t)group_offsets[g], (int32_t)m});
                n_edges += m - 1;
            }
            return 0;
        },
        [&](int32_t id) {
            if (ctx->lens[(size_t)id] > 65535)
                return fail(LCSGPU_E_UNSUPPORTED, "sequence %d is longer than 65535 residues: the batched MST keeps 16-bit LCS values", id);
            if (!triangle_orientation && ctx->quirk[(size_t)id])
                return fail(LCSGPU_E_UNSUPPORTED, "sequence %d is orientation sensitive: MSTPrim's distances depend on which endpoint is "
                                                  "the ref, the triangle does not hold them (use lcsgpu_mst_prim)", id);
            return 0;
        });
    if (rc || jobs.empty()) return rc;
    if (!out_edges) return fail(LCSGPU_E_INVALID, "NULL out_edges");
    // The LCS values of (cur, v) from the group's expanded m x m square (one contiguous row per step) or -- LCSGPU_TUNE
    // mst_batch_square=0 -- from the packed triangle as it is (v > cur: a strided 2-byte gather).  A step is latency more
    // than bytes, so the square gains little: the Prim launch with its expansion 0.378 against 0.385 ms at m = 256, 1.95
    // against 2.08 ms at 1000, 17.6 against 19.3 ms at 4096 (profiles/batch_trees.txt) -- faster at every size from 200 up,
    // for twice the triangles' memory again.
    static const int use_square = tune_int("mst_batch_square", 1);

    GroupCall call(ctx);
    Lane& L = call.L;
    rc = call.triangles(ids, group_offsets, n_groups, "MST", jobs);
    if (rc) return rc;
    const int64_t n_total = group_offsets[n_groups];
    std::vector<int64_t> row0(jobs.size() + 1, 0);
    int32_t max_m = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        lcsgpu::GroupPrimJob& job = jobs[j];
        job.sq0 = sq_elems;
        sq_elems += (int64_t)job.m * job.m;
        row0[j + 1] = row0[j] + job.m;
        max_m = std::max(max_m, job.m);
    }
    const size_t o_jobs = 0, o_row0 = o_jobs + a256(jobs.size() * sizeof(lcsgpu::GroupPrimJob)), o_ids = o_row0 + a256(row0.size() * 8),
                 o_edges = o_ids + a256((size_t)n_total * 4), o_sq = o_edges + a256((size_t)n_edges * sizeof(lcsgpu_mst_edge)),
                 total = o_sq + (use_square ? a256((size_t)sq_elems * 2) : 0);
    rc = reserve_big(ctx, L.d_work, total, "the batched MST's tables");
    if (rc) return rc;
    char* base = (char*)L.d_work.p;
    HIP_TRY(hipMemcpyAsync(base + o_jobs, jobs.data(), jobs.size() * sizeof(lcsgpu::GroupPrimJob), hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_row0, row0.data(), row0.size() * 8, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_ids, ids, (size_t)n_total * 4, hipMemcpyHostToDevice, L.stream));
    lcsgpu::GroupPrimArgs a{};
    a.tri = (const uint16_t*)L.d_out.p;
    a.sq = use_square ? (uint16_t*)(base + o_sq) : nullptr;
    a.jobs = (const lcsgpu::GroupPrimJob*)(base + o_jobs);
    a.row0 = (const int64_t*)(base + o_row0);
    a.ids = (const int32_t*)(base + o_ids);
    a.lens = (const uint32_t*)ctx->d_lens.p;
    a.pow_table = (const double*)ctx->d_pow.p;
    a.edges = (lcsgpu::MstEdge*)(base + o_edges);
    a.total_rows = row0.back();
    a.pow_n = (int32_t)(2 * (size_t)ctx->max_len + 1);
    a.n_jobs = (int32_t)jobs.size();
    a.kind = distance_kind;
    a.max_m = max_m;
    if (const hipError_t e = lcsgpu::launch_group_prim(a, L.stream))
        return fail(LCSGPU_E_HIP, "the batched MST's launch failed: %s", hipGetErrorString(e));
    static_assert(sizeof(lcsgpu_mst_edge) == sizeof(lcsgpu::MstEdge), "edge records");
    return call.finish(use_square ? 2 : 1, [&] {
        HIP_TRY(hipMemcpy(out_edges, base + o_edges, (size_t)n_edges * sizeof(lcsgpu_mst_edge), hipMemcpyDeviceToHost));
        return LCSGPU_OK;
    });
}

// UPGMA of many id lists: the lists' triangles by the launches of lcsgpu_lcs_triangles_batch, then per slice of lists a
// launch pair (upgma_group_kernels.hip): the float squares with the rows' initial keys, and a workgroup per list that runs
// the list's merges, longest lists first.
static int upgma_batch_impl(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, int distance_kind,
                            int modified, int32_t* out_left, int32_t* out_right, int32_t* out_status)
{
    // everything that refuses comes first: nothing is computed, the outputs stay as they are
    std::vector<lcsgpu::GroupUpgmaJob> jobs;
    int64_t n_nodes = 0;
    int rc = check_groups(
        ctx, ids, group_offsets, n_groups, distance_kind,
        [&](int32_t g, int64_t m) {
            if (m > LCSGPU_UPGMA_BATCH_MAX_MEMBERS)
                return fail(LCSGPU_E_UNSUPPORTED, "group %d has %lld members: the batched UPGMA handles at most %d (use lcsgpu_upgma)", g,
                            (long long)m, LCSGPU_UPGMA_BATCH_MAX_MEMBERS);
            if (m >= 2) {
                jobs.push_back(lcsgpu::GroupUpgmaJob{(int64_t)g /* the group, until its triangle's place is known */, 0, n_nodes,
                                                     (int32_t)group_offsets[g], (int32_t)m, g, 0});
                n_nodes += m - 1;
            }
            return 0;
        },
        [&](int32_t id) {
            // (orientation-sensitive members are served: the triangle's orientation, ref = the later member, IS
            // UPGMA::computeDistances's)
            if (ctx->lens[(size_t)id] > 65535)
                return fail(LCSGPU_E_UNSUPPORTED, "sequence %d is longer than 65535 residues: the batched UPGMA keeps 16-bit LCS values", id);
            return 0;
        });
    if (rc || n_groups == 0) return rc;
    if (!out_status) return fail(LCSGPU_E_INVALID, "NULL out_status");
    if (n_nodes > 0 && (!out_left || !out_right)) return fail(LCSGPU_E_INVALID, "NULL out_left / out_right");
    if (jobs.empty()) {
        std::fill(out_status, out_status + n_groups, 0);
        return LCSGPU_OK;
    }
    // the float squares of a launch pair: at most this many MB (a slice always holds at least one group)
    static const int slice_mb = std::max(1, tune_int("upgma_group_mb", 4096));

    GroupCall call(ctx);
    Lane& L = call.L;
    rc = call.triangles(ids, group_offsets, n_groups, "UPGMA", jobs);
    if (rc) return rc;
    const int64_t n_total = group_offsets[n_groups];
    struct Slice { size_t job0, n_jobs, row_at; int64_t rows, sq_elems; int32_t max_m; };
    std::vector<Slice> slices;
    std::vector<int64_t> row0; // per slice: the prefix sums of m over its jobs, one slice after the other
    const int64_t slice_elems = (int64_t)slice_mb * (1 << 20) / 4;
    int64_t max_sq = 0, max_rows = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        lcsgpu::GroupUpgmaJob& job = jobs[j];
        const int64_t sq = (int64_t)job.m * job.m;
        if (slices.empty() || slices.back().sq_elems + sq > slice_elems) {
            slices.push_back(Slice{j, 0, row0.size(), 0, 0, job.m});
            row0.push_back(0);
        }
        Slice& s = slices.back();
        job.sq0 = s.sq_elems;
        s.sq_elems += sq;
        s.rows += job.m;
        ++s.n_jobs;
        row0.push_back(s.rows);
        max_sq = std::max(max_sq, s.sq_elems);
        max_rows = std::max(max_rows, s.rows);
    }
    const size_t o_jobs = 0, o_row0 = o_jobs + a256(jobs.size() * sizeof(lcsgpu::GroupUpgmaJob)), o_ids = o_row0 + a256(row0.size() * 8),
                 o_left = o_ids + a256((size_t)n_total * 4), o_right = o_left + a256((size_t)n_nodes * 4),
                 o_status = o_right + a256((size_t)n_nodes * 4), o_min = o_status + a256((size_t)n_groups * 4),
                 o_near = o_min + a256((size_t)max_rows * 4), o_sq = o_near + a256((size_t)max_rows * 4),
                 total = o_sq + a256((size_t)max_sq * 4);
    rc = reserve_big(ctx, L.d_work, total, "the batched UPGMA's tables and squares");
    if (rc) return rc;
    char* base = (char*)L.d_work.p;
    HIP_TRY(hipMemcpyAsync(base + o_jobs, jobs.data(), jobs.size() * sizeof(lcsgpu::GroupUpgmaJob), hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_row0, row0.data(), row0.size() * 8, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_ids, ids, (size_t)n_total * 4, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemsetAsync(base + o_status, 0, (size_t)n_groups * 4, L.stream));
    for (const Slice& s : slices) {
        lcsgpu::GroupUpgmaArgs a{};
        a.tri = (const uint16_t*)L.d_out.p;
        a.sq = (float*)(base + o_sq);
        a.jobs = (const lcsgpu::GroupUpgmaJob*)(base + o_jobs) + s.job0;
        a.row0 = (const int64_t*)(base + o_row0) + s.row_at;
        a.ids = (const int32_t*)(base + o_ids);
        a.lens = (const uint32_t*)ctx->d_lens.p;
        a.pow_f32 = (const float*)ctx->d_powf.p;
        a.row_min = (float*)(base + o_min);
        a.row_near = (int32_t*)(base + o_near);
        a.left = (int32_t*)(base + o_left);
        a.right = (int32_t*)(base + o_right);
        a.status = (int32_t*)(base + o_status);
        a.total_rows = s.rows;
        a.n_jobs = (int32_t)s.n_jobs;
        a.kind = distance_kind;
        a.modified = modified ? 1 : 0;
        a.max_m = s.max_m;
        if (const hipError_t e = lcsgpu::launch_group_upgma(a, L.stream))
            return fail(LCSGPU_E_HIP, "the batched UPGMA's launch failed: %s", hipGetErrorString(e));
    }
    return call.finish(2 * (int)slices.size(), [&] { // left | right | status are neighbours in the work buffer: one copy, then three
        std::vector<char> back(o_min - o_left);
        HIP_TRY(hipMemcpy(back.data(), base + o_left, back.size(), hipMemcpyDeviceToHost));
        memcpy(out_left, back.data(), (size_t)n_nodes * 4);
        memcpy(out_right, back.data() + (o_right - o_left), (size_t)n_nodes * 4);
        memcpy(out_status, back.data() + (o_status - o_left), (size_t)n_groups * 4);
        return LCSGPU_OK;
    });
}

// Neighbour joining of many id lists: the lists' triangles by the launches of lcsgpu_lcs_triangles_batch, then per slice of
// lists the launches of nj_group_kernels.hip: the float triangles with the rows' initial sums, and a workgroup per list
// that runs the list's merges, longest lists first.
static int nj_batch_impl(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, int distance_kind,
                         int32_t* out_left, int32_t* out_right, int32_t* out_status)
{
    // everything that refuses comes first: nothing is computed, the outputs stay as they are
    std::vector<lcsgpu::GroupNjJob> jobs;
    int64_t n_nodes = 0;
    int rc = check_groups(
        ctx, ids, group_offsets, n_groups, distance_kind,
        [&](int32_t g, int64_t m) {
            if (m > LCSGPU_NJ_BATCH_MAX_MEMBERS)
                return fail(LCSGPU_E_UNSUPPORTED, "group %d has %lld members: the batched NJ handles at most %d (use lcsgpu_nj)", g,
                            (long long)m, LCSGPU_NJ_BATCH_MAX_MEMBERS);
            if (m >= 2) {
                jobs.push_back(lcsgpu::GroupNjJob{(int64_t)g /* the group, until its triangle's place is known */, 0, n_nodes,
                                                  (int32_t)group_offsets[g], (int32_t)m, g, 0});
                n_nodes += m - 1;
            }
            return 0;
        },
        [&](int32_t id) {
            // (orientation-sensitive members are served: the triangle's orientation, ref = the later member, IS
            // calculateDistanceMatrix's)
            if (ctx->lens[(size_t)id] > 65535)
                return fail(LCSGPU_E_UNSUPPORTED, "sequence %d is longer than 65535 residues: the batched NJ keeps 16-bit LCS values", id);
            return 0;
        });
    if (rc || n_groups == 0) return rc;
    if (!out_status) return fail(LCSGPU_E_INVALID, "NULL out_status");
    if (n_nodes > 0 && (!out_left || !out_right)) return fail(LCSGPU_E_INVALID, "NULL out_left / out_right");
    if (jobs.empty()) {
        std::fill(out_status, out_status + n_groups, 0);
        return LCSGPU_OK;
    }
    // the float triangles of a slice: at most this many MB (a slice always holds at least one group)
    const int slice_mb = std::max(1, tune_int("nj_group_mb", 2048));
    // 256 threads below NJ_GROUP_WIDE_AT members, 1024 from there on (profiles/batch_nj.txt); nj_group_threads forces one
    // (neither is cached: tests switch them inside one process)
    const int forced_threads = tune_int("nj_group_threads", 0);
    const int wide_at = forced_threads == 256 ? LCSGPU_NJ_BATCH_MAX_MEMBERS + 1 : forced_threads == 1024 ? 0 : lcsgpu::NJ_GROUP_WIDE_AT;

    GroupCall call(ctx);
    Lane& L = call.L;
    rc = call.triangles(ids, group_offsets, n_groups, "NJ", jobs);
    if (rc) return rc;
    const int64_t n_total = group_offsets[n_groups];
    struct Slice { size_t job0, n_jobs, row_at; int64_t rows, elems; int32_t max_m, n_wide, narrow_m; };
    std::vector<Slice> slices;
    std::vector<int64_t> row0; // per slice: the prefix sums of m over its jobs, one slice after the other
    const int64_t slice_elems = (int64_t)slice_mb * (1 << 20) / 4;
    int64_t max_elems = 0, max_rows = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        lcsgpu::GroupNjJob& job = jobs[j];
        // n_wide / narrow_m below, and the LDS of a launch (its first job's m), rely on GroupCall::triangles' order
        if (j > 0 && job.m > jobs[j - 1].m) return fail(LCSGPU_E_STATE, "the batched NJ's jobs are not longest first");
        const int64_t elems = (int64_t)job.m * (job.m - 1) / 2;
        if (slices.empty() || slices.back().elems + elems > slice_elems) {
            slices.push_back(Slice{j, 0, row0.size(), 0, 0, job.m, 0, 0});
            row0.push_back(0);
        }
        Slice& s = slices.back();
        job.f0 = s.elems;
        s.elems += elems;
        s.rows += job.m;
        if (job.m >= wide_at) ++s.n_wide; // (longest first: the wide jobs are the slice's first)
        else if (s.narrow_m == 0) s.narrow_m = job.m;
        ++s.n_jobs;
        row0.push_back(s.rows);
        max_elems = std::max(max_elems, s.elems);
        max_rows = std::max(max_rows, s.rows);
    }
    const size_t o_jobs = 0, o_row0 = o_jobs + a256(jobs.size() * sizeof(lcsgpu::GroupNjJob)), o_ids = o_row0 + a256(row0.size() * 8),
                 o_left = o_ids + a256((size_t)n_total * 4), o_right = o_left + a256((size_t)n_nodes * 4),
                 o_status = o_right + a256((size_t)n_nodes * 4), o_sum = o_status + a256((size_t)n_groups * 4),
                 o_dist = o_sum + a256((size_t)max_rows * 4), total = o_dist + a256((size_t)max_elems * 4);
    rc = reserve_big(ctx, L.d_work, total, "the batched NJ's tables and float triangles");
    if (rc) return rc;
    char* base = (char*)L.d_work.p;
    HIP_TRY(hipMemcpyAsync(base + o_jobs, jobs.data(), jobs.size() * sizeof(lcsgpu::GroupNjJob), hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_row0, row0.data(), row0.size() * 8, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_ids, ids, (size_t)n_total * 4, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemsetAsync(base + o_status, 0, (size_t)n_groups * 4, L.stream));
    int launches = 0;
    for (const Slice& s : slices) {
        lcsgpu::GroupNjArgs a{};
        a.tri = (const uint16_t*)L.d_out.p;
        a.dist = (float*)(base + o_dist);
        a.jobs = (const lcsgpu::GroupNjJob*)(base + o_jobs) + s.job0;
        a.row0 = (const int64_t*)(base + o_row0) + s.row_at;
        a.ids = (const int32_t*)(base + o_ids);
        a.lens = (const uint32_t*)ctx->d_lens.p;
        a.pow_f32 = (const float*)ctx->d_powf.p;
        a.row_sum = (float*)(base + o_sum);
        a.left = (int32_t*)(base + o_left);
        a.right = (int32_t*)(base + o_right);
        a.status = (int32_t*)(base + o_status);
        a.total_rows = s.rows;
        a.n_jobs = (int32_t)s.n_jobs;
        a.kind = distance_kind;
        a.max_m = s.max_m;
        a.n_wide = s.n_wide;
        a.narrow_m = s.narrow_m;
        if (const hipError_t e = lcsgpu::launch_group_nj(a, L.stream))
            return fail(LCSGPU_E_HIP, "the batched NJ's launch failed: %s", hipGetErrorString(e));
        launches += lcsgpu::group_nj_launches(a);
    }
    return call.finish(launches, [&] { // left | right | status are neighbours in the work buffer: one copy, then three
        std::vector<char> back(o_sum - o_left);
        HIP_TRY(hipMemcpy(back.data(), base + o_left, back.size(), hipMemcpyDeviceToHost));
        memcpy(out_left, back.data(), (size_t)n_nodes * 4);
        memcpy(out_right, back.data() + (o_right - o_left), (size_t)n_nodes * 4);
        memcpy(out_status, back.data() + (o_status - o_left), (size_t)n_groups * 4);
        return LCSGPU_OK;
    });
}

// -dist_export for many id lists in one call: the lists' triangles (lower form; the launches of lcsgpu_lcs_triangles_batch) or
// m x m rectangles (square form) stay in the lane's result buffer, the job-table form of the formatter (text_kernels.hip,
// tables from text_plan.h) turns all rows of all lists into text: lengths and scans, the lists' offsets and the total to the
// host -- the call's one synchronisation in the middle --, the exactly sized output, the write pass, one copy back.
static int dist_text_batch_impl(lcsgpu_ctx* ctx, const char* names, const uint64_t* name_offsets, const int32_t* ids,
                                const int64_t* group_offsets, int32_t n_groups, int distance_kind, int flags, const char** text,
                                uint64_t* text_offsets)
{
    const bool pid = (flags & LCSGPU_TEXT_PID) != 0, square = (flags & LCSGPU_TEXT_SQUARE) != 0;
    // everything that refuses comes first: nothing is computed, the outputs stay as they are
    if (!ctx) return fail(LCSGPU_E_INVALID, "NULL ctx");
    if (!name_offsets || !text || !text_offsets) return fail(LCSGPU_E_INVALID, "NULL argument");
    int rc = check_groups(
        ctx, ids, group_offsets, n_groups, pid ? LCSGPU_DIST_INDEL075_DIV_LCS : distance_kind,
        [&](int32_t g, int64_t m) {
            if (m > LCSGPU_DIST_TEXT_BATCH_MAX_MEMBERS)
                return fail(LCSGPU_E_UNSUPPORTED, "group %d has %lld members: the batched text handles at most %d (use lcsgpu_dist_text_begin)", g,
                            (long long)m, LCSGPU_DIST_TEXT_BATCH_MAX_MEMBERS);
            return 0;
        },
        [&](int32_t id) {
            if (ctx->lens[(size_t)id] > 65535)
                return fail(LCSGPU_E_UNSUPPORTED, "sequence %d is longer than 65535 residues: the batched text keeps 16-bit LCS values", id);
            return 0;
        });
    if (rc) return rc;
    const int32_t n = ctx->n;
    for (int32_t i = 0; i < n; ++i)
        if (name_offsets[i + 1] < name_offsets[i]) return fail(LCSGPU_E_INVALID, "name offsets not monotone at %d", i);
    const uint64_t name_base = n > 0 ? name_offsets[0] : 0, name_bytes = n > 0 ? name_offsets[n] - name_base : 0;
    if (name_bytes > 0 && !names) return fail(LCSGPU_E_INVALID, "NULL names");
    lcsgpu_impl::TextPlan plan;
    if (!plan_text(group_offsets, n_groups, square, plan)) return fail(LCSGPU_E_INVALID, "batch too large");
    const int64_t n_rows = (int64_t)plan.rows.size() - 1, n_jobs = (int64_t)plan.job_row.size(), n_total = n_rows;

    HIP_TRY(hipSetDevice(ctx->device));
    PinBuf& h_text = ctx->h_batch_text[ctx->batch_text_next]; // the buffer of the call before the last one: its text ends here
    if (n_rows == 0) { // no list, or empty lists only
        if (h_text.reserve(16) != hipSuccess) return fail(LCSGPU_E_NOMEM, "the batched text: no pinned host memory");
        ctx->batch_text_next ^= 1;
        *text = (const char*)h_text.p;
        std::fill(text_offsets, text_offsets + n_groups + 1, (uint64_t)0);
        return LCSGPU_OK;
    }
    std::vector<uint64_t> name_off(name_offsets, name_offsets + n + 1);
    for (uint64_t& o : name_off) o -= name_base;

    GroupCall call(ctx);
    Lane& L = call.L;
    // (not GroupCall::triangles: a call whose lists hold no pair still has its "name\n" rows to make)
    rc = batch_triangles_to_device(ctx, L, ids, group_offsets, n_groups, 2, call.tri_base, &call.count, &call.had_long, [&] { call.hold.lock(); }, square);
    if (rc) return rc;
    if (call.count <= 0) { // nothing was launched: the text kernels are the call's own
        call.hold.lock();
        L.last_launches = 0;
        HIP_TRY(hipEventRecord(L.ev_start, L.stream));
        L.timing_valid = true;
    } else if (call.tri_base != plan.list_src0)
        return fail(LCSGPU_E_STATE, "the batched text's plan and its LCS launches disagree about the lists' places");
    const size_t o_rows = 0, o_job = o_rows + a256(plan.rows.size() * sizeof(lcsgpu_impl::TextRow)), o_ids = o_job + a256((size_t)n_jobs * 4),
                 o_lrow = o_ids + a256((size_t)n_total * 4), o_names = o_lrow + a256(((size_t)n_groups + 1) * 8),
                 o_noff = o_names + a256((size_t)name_bytes + 16), o_seg = o_noff + a256(((size_t)n + 1) * 8),
                 o_rlen = o_seg + a256((size_t)n_jobs * 4), o_rstart = o_rlen + a256((size_t)n_rows * 4),
                 o_lstart = o_rstart + a256(((size_t)n_rows + 1) * 8), total = o_lstart + a256(((size_t)n_groups + 1) * 8);
    rc = reserve_big(ctx, L.d_work, total, "the batched text's tables");
    if (rc) return rc;
    HIP_TRY(L.h_small.reserve(((size_t)n_groups + 1) * 8));
    char* base = (char*)L.d_work.p;
    HIP_TRY(hipMemcpyAsync(base + o_rows, plan.rows.data(), plan.rows.size() * sizeof(lcsgpu_impl::TextRow), hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_job, plan.job_row.data(), (size_t)n_jobs * 4, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_ids, ids, (size_t)n_total * 4, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_lrow, plan.list_row0.data(), ((size_t)n_groups + 1) * 8, hipMemcpyHostToDevice, L.stream));
    if (name_bytes) HIP_TRY(hipMemcpyAsync(base + o_names, names + name_base, (size_t)name_bytes, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_noff, name_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, L.stream));
    lcsgpu::TextGroupArgs g{};
    g.lcs = (const uint16_t*)L.d_out.p;
    g.rows = (const lcsgpu_impl::TextRow*)(base + o_rows);
    g.job_row = (const int32_t*)(base + o_job);
    g.ids = (const int32_t*)(base + o_ids);
    g.list_row0 = (const int64_t*)(base + o_lrow);
    g.lens = (const uint32_t*)ctx->d_lens.p;
    g.pow_f64 = (const double*)ctx->d_pow.p;
    g.names = (const char*)(base + o_names);
    g.name_off = (const uint64_t*)(base + o_noff);
    g.seg_len = (uint32_t*)(base + o_seg);
    g.row_len = (uint32_t*)(base + o_rlen);
    g.row_start = (unsigned long long*)(base + o_rstart);
    g.list_start = (unsigned long long*)(base + o_lstart);
    g.kind = pid ? 2 : distance_kind;
    g.n_rows = (int32_t)n_rows;
    g.n_jobs = (int32_t)n_jobs;
    g.n_groups = n_groups;
    if (const hipError_t e = lcsgpu::launch_text_group_lengths(g, L.stream))
        return fail(LCSGPU_E_HIP, "the batched text's length launches failed: %s", hipGetErrorString(e));
    // the lists' offsets and the total: what sizes the output exactly (39 B per value, the worst case, would forbid the
    // chunks the callers make)
    HIP_TRY(hipMemcpyAsync(L.h_small.p, g.list_start, ((size_t)n_groups + 1) * 8, hipMemcpyDeviceToHost, L.stream));
    HIP_TRY(hipEventRecord(L.ev_done, L.stream));
    HIP_TRY(hipEventSynchronize(L.ev_done));
    const uint64_t* list_start = (const uint64_t*)L.h_small.p;
    const uint64_t bytes = list_start[n_groups];
    rc = reserve_big(ctx, ctx->d_batch_text, (size_t)bytes + 64, "the batched text");
    if (rc) return rc;
    if (h_text.reserve((size_t)bytes + 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LCSGPU_E_NOMEM, "the batched text: %llu bytes of pinned host memory", (unsigned long long)bytes);
    }
    g.out = (char*)ctx->d_batch_text.p;
    if (const hipError_t e = lcsgpu::launch_text_group_write(g, L.stream))
        return fail(LCSGPU_E_HIP, "the batched text's write launch failed: %s", hipGetErrorString(e));
    return call.finish(5, [&] {
        HIP_TRY(hipMemcpy(h_text.p, ctx->d_batch_text.p, (size_t)bytes, hipMemcpyDeviceToHost));
        ctx->batch_text_next ^= 1;
        *text = (const char*)h_text.p;
        std::copy(list_start, list_start + n_groups + 1, text_offsets);
        return LCSGPU_OK;
    });
}

static int assign_seeds_impl(lcsgpu_ctx* ctx, const int32_t* seed_ids, int32_t n_seeds, const int32_t* col_ids, int32_t n_cols,
                             int distance_kind, int32_t first_k, float* dist, int32_t* assign)
{
    if (!ctx) return fail(LCSGPU_E_INVALID, "NULL ctx");
    if (ctx->n < 0) return fail(LCSGPU_E_STATE, "no sequence set uploaded");
    if (!valid_kind(distance_kind)) return fail(LCSGPU_E_INVALID, "unknown distance kind %d", distance_kind);
    if (n_seeds < 0 || n_cols < 0) return fail(LCSGPU_E_INVALID, "negative count");
    if (n_seeds == 0 || n_cols == 0) return LCSGPU_OK;
    if (!seed_ids || !col_ids || !dist || !assign) return fail(LCSGPU_E_INVALID, "NULL argument");
    for (int32_t r = 0; r < n_seeds; ++r)
        if (seed_ids[r] < 0 || seed_ids[r] >= ctx->n) return fail(LCSGPU_E_INVALID, "seed id %d out of range", seed_ids[r]);
    LaneGuard guard(ctx, LaneGuard::ANY);
    Lane& L = guard.lane();
    HIP_TRY(hipSetDevice(ctx->device));
    const int elem = ctx->max_len > 65535 ? 4 : 2;
    // column chunks: the LCS rectangle of a chunk stays below 256 MB
    const int32_t chunk = (int32_t)std::max<int64_t>(4096, std::min<int64_t>(n_cols, ((int64_t)256 << 20) / ((int64_t)n_seeds * elem)));
    const size_t o_seeds = 0, o_cols = o_seeds + a256((size_t)n_seeds * 4), o_dist = o_cols + a256((size_t)chunk * 4),
                 o_assign = o_dist + a256((size_t)chunk * 4), total = o_assign + a256((size_t)chunk * 4);
    HIP_TRY(L.d_work.reserve(total));
    HIP_TRY(L.d_out.reserve((size_t)n_seeds * chunk * elem));
    char* base = (char*)L.d_work.p;
    HIP_TRY(hipMemcpyAsync(base + o_seeds, seed_ids, (size_t)n_seeds * 4, hipMemcpyHostToDevice, L.stream));
    double ms = 0;
    int launches = 0;
    for (int32_t c0 = 0; c0 < n_cols; c0 += chunk) {
        const int32_t cn = std::min(chunk, n_cols - c0);
        HIP_TRY(hipMemcpyAsync(base + o_cols, col_ids + c0, (size_t)cn * 4, hipMemcpyHostToDevice, L.stream));
        HIP_TRY(hipMemcpyAsync(base + o_dist, dist + c0, (size_t)cn * 4, hipMemcpyHostToDevice, L.stream));
        HIP_TRY(hipMemcpyAsync(base + o_assign, assign + c0, (size_t)cn * 4, hipMemcpyHostToDevice, L.stream));
        int rc = run_rows(ctx, L, lcsgpu::MODE_RECT, seed_ids, 0, n_seeds, col_ids + c0, 0, cn, L.d_out.p, cn, 0, elem);
        if (rc) return rc;
        HIP_TRY(lcsgpu::launch_assign_seeds(L.d_out.p, elem, cn, (const int32_t*)(base + o_seeds), n_seeds,
                                            (const int32_t*)(base + o_cols), cn, (const uint32_t*)ctx->d_lens.p,
                                            (const float*)ctx->d_powf.p, distance_kind, first_k, (float*)(base + o_dist),
                                            (int32_t*)(base + o_assign), L.stream));
        HIP_TRY(hipMemcpyAsync(dist + c0, base + o_dist, (size_t)cn * 4, hipMemcpyDeviceToHost, L.stream));
        HIP_TRY(hipMemcpyAsync(assign + c0, base + o_assign, (size_t)cn * 4, hipMemcpyDeviceToHost, L.stream));
        HIP_TRY(hipEventRecord(L.ev_done, L.stream));
        HIP_TRY(hipEventSynchronize(L.ev_done));
        finish_host_call(ctx, L);
        ms += g_last.ms;
        launches += g_last.launches;
    }
    g_last.ms = ms;
    g_last.launches = launches;
    return LCSGPU_OK;
}

static int assign_seeds_batch_impl(lcsgpu_ctx* ctx, const int32_t* seed_ids, const int64_t* seed_offsets, const int32_t* col_ids,
                                   const int64_t* col_offsets, int32_t n_jobs, int distance_kind, float* dist, int32_t* assign)
{
    if (!ctx) return fail(LCSGPU_E_INVALID, "NULL ctx");
    if (ctx->n < 0) return fail(LCSGPU_E_STATE, "no sequence set uploaded");
    if (!valid_kind(distance_kind)) return fail(LCSGPU_E_INVALID, "unknown distance kind %d", distance_kind);
    if (n_jobs < 0 || (n_jobs > 0 && (!seed_offsets || !col_offsets))) return fail(LCSGPU_E_INVALID, "bad job tables");
    if (n_jobs == 0) return LCSGPU_OK;
    if (seed_offsets[0] != 0 || col_offsets[0] != 0) return fail(LCSGPU_E_INVALID, "offsets must start at 0");
    for (int32_t j = 0; j < n_jobs; ++j)
        if (seed_offsets[j + 1] < seed_offsets[j] || col_offsets[j + 1] < col_offsets[j] || seed_offsets[j + 1] - seed_offsets[j] > 0x7fffffff)
            return fail(LCSGPU_E_INVALID, "offsets not ascending at job %d", j);
    const int64_t n_seeds_all = seed_offsets[n_jobs], n_cols_all = col_offsets[n_jobs];
    if (n_cols_all == 0) return LCSGPU_OK;
    if (!col_ids || !dist || !assign || (n_seeds_all > 0 && !seed_ids)) return fail(LCSGPU_E_INVALID, "NULL argument");
    if (n_seeds_all > 0x7fffffff) return fail(LCSGPU_E_INVALID, "too many seeds");
    bool any_long = false;
    for (int64_t s = 0; s < n_seeds_all; ++s) {
        if (seed_ids[s] < 0 || seed_ids[s] >= ctx->n) return fail(LCSGPU_E_INVALID, "seed id %d out of range", seed_ids[s]);
        any_long |= ctx->lens[seed_ids[s]] > 2048;
    }
    for (int64_t c = 0; c < n_cols_all; ++c)
        if (col_ids[c] < 0 || col_ids[c] >= ctx->n) return fail(LCSGPU_E_INVALID, "col id %d out of range", col_ids[c]);
    if (any_long) { // the long-ref kernel keeps its 2-D grid: evaluation by evaluation
        for (int32_t j = 0; j < n_jobs; ++j) {
            const int64_t c0 = col_offsets[j], nc = col_offsets[j + 1] - c0;
            if (nc > 0x7fffffff) return fail(LCSGPU_E_INVALID, "too many columns in job %d", j);
            for (int64_t c = 0; c < nc; ++c) {
                dist[c0 + c] = std::numeric_limits<float>::infinity();
                assign[c0 + c] = 0;
            }
            int rc = assign_seeds_impl(ctx, seed_ids + seed_offsets[j], (int32_t)(seed_offsets[j + 1] - seed_offsets[j]), col_ids + c0, (int32_t)nc,
                                       distance_kind, 0, dist + c0, assign + c0);
            if (rc) return rc;
        }
        return LCSGPU_OK;
    }
    LaneGuard guard(ctx, LaneGuard::FRONT);
    Lane& L = guard.lane();
    HIP_TRY(hipSetDevice(ctx->device));
    const int elem = ctx->max_len > 65535 ? 4 : 2;
    // pieces = (job, column range), taken in order, so that a launch covers one contiguous range of the caller's columns;
    // a launch's rectangles stay below `cap` bytes
    const int64_t cap = (int64_t)std::max(1, tune_int("assign_batch_kb", 2048 << 10)) << 10;
    struct Piece { int32_t job; int64_t c0, c1; };
    std::vector<Piece> pieces;
    for (int32_t j = 0; j < n_jobs; ++j) {
        const int64_t ns = seed_offsets[j + 1] - seed_offsets[j], c0 = col_offsets[j], c1 = col_offsets[j + 1];
        if (c1 == c0) continue;
        if (ns == 0) { // no seed: nothing beats +inf
            for (int64_t c = c0; c < c1; ++c) { dist[c] = std::numeric_limits<float>::infinity(); assign[c] = 0; }
            continue;
        }
        const int64_t step = std::max<int64_t>(256, (cap / (ns * elem)) & ~(int64_t)255);
        for (int64_t a = c0; a < c1; a += step) pieces.push_back(Piece{j, a, std::min(c1, a + step)});
    }
    HIP_TRY(L.d_draws.reserve((size_t)n_seeds_all * 4 + 16)); // (the lane's spare buffer: the seeds of all jobs)
    HIP_TRY(hipMemcpyAsync(L.d_draws.p, seed_ids, (size_t)n_seeds_all * 4, hipMemcpyHostToDevice, L.stream));
    double ms = 0;
    int launches = 0;
    std::vector<JobRef> refs;
    std::vector<JobBucket> buckets;
    for (size_t p0 = 0; p0 < pieces.size();) {
        // the launch: pieces [p0, p1) as far as their columns are contiguous and the rectangles fit
        size_t p1 = p0;
        int64_t bytes = 0;
        while (p1 < pieces.size()) {
            const Piece& pc = pieces[p1];
            const int64_t ns = seed_offsets[pc.job + 1] - seed_offsets[pc.job];
            const int64_t b = ns * (pc.c1 - pc.c0) * elem;
            if (p1 > p0 && (bytes + b > cap || pieces[p1 - 1].c1 != pc.c0 || pc.c1 - pieces[p0].c0 > 0x7fffff00)) break;
            bytes += b;
            ++p1;
        }
        const int64_t C0 = pieces[p0].c0, C1 = pieces[p1 - 1].c1, nc = C1 - C0;
        if (nc > 0x7fffff00) return fail(LCSGPU_E_INVALID, "a job's column range is too long for one launch");
        const int32_t np = (int32_t)(p1 - p0);
        // the refs: every seed of every piece, a row of the piece's rectangle each; columns are relative to the launch's first
        std::vector<lcsgpu::AssignPiece> table((size_t)np);
        refs.clear();
        int64_t out_at = 0;
        for (size_t p = p0; p < p1; ++p) {
            const Piece& pc = pieces[p];
            const int64_t s0 = seed_offsets[pc.job], ns = seed_offsets[pc.job + 1] - s0, w = pc.c1 - pc.c0;
            table[p - p0] = lcsgpu::AssignPiece{out_at, (int32_t)(pc.c0 - C0), (int32_t)w, (int32_t)s0, (int32_t)ns};
            for (int64_t r = 0; r < ns; ++r) {
                const int32_t id = seed_ids[s0 + r];
                const uint8_t c = ctx->ref_class[(size_t)id];
                const bool q = (c & 0x80) != 0;
                refs.push_back(JobRef{id, (int32_t)(p - p0), (int32_t)(pc.c0 - C0), pc.c1 - C0, out_at + r * w,
                                      q ? 0.0 : (double)((w + 255) / 256) / lcsgpu::refs_per_block_for(c, false, 1, 1), c,
                                      (uint8_t)(q ? lcsgpu::quirk_h_class(ctx->lens[id]) : 0), false});
            }
            out_at += ns * w;
        }
        if (!plan_jobs(refs, (long)std::max<int64_t>(1, nc / 256 / std::max(1, np)), lcsgpu::refs_per_block_for, buckets))
            return fail(LCSGPU_E_INVALID, "batch too large");
        PlanLayout lay;
        int rc = stage_job_tables(L, buckets, table.data(), (size_t)np * sizeof(lcsgpu::AssignPiece), lay);
        if (rc) return rc;
        // columns, distances, assignments of the launch
        const size_t o_cols = 0, o_dist = o_cols + a256((size_t)nc * 4), o_assign = o_dist + a256((size_t)nc * 4), work = o_assign + a256((size_t)nc * 4);
        HIP_TRY(L.d_work.reserve(work));
        rc = reserve_big(ctx, L.d_out, (size_t)out_at * elem, "assign_seeds_batch rectangles");
        if (rc) return rc;
        char* base = (char*)L.d_work.p;
        HIP_TRY(hipMemcpyAsync(base + o_cols, col_ids + C0, (size_t)nc * 4, hipMemcpyHostToDevice, L.stream));
        rc = launch_job_tables(ctx, L, buckets, lay, lcsgpu::MODE_RECT, (const int32_t*)(base + o_cols), nc, elem);
        if (rc) return rc;
        HIP_TRY(lcsgpu::launch_assign_seeds_batch(L.d_out.p, elem, (const lcsgpu::AssignPiece*)L.d_plan.p /* the plan buffer's first table */, np,
                                                  (const int32_t*)L.d_draws.p, (const int32_t*)(base + o_cols), nc, (const uint32_t*)ctx->d_lens.p,
                                                  (const float*)ctx->d_powf.p, distance_kind, (float*)(base + o_dist), (int32_t*)(base + o_assign), L.stream));
        HIP_TRY(hipMemcpyAsync(dist + C0, base + o_dist, (size_t)nc * 4, hipMemcpyDeviceToHost, L.stream));
        HIP_TRY(hipMemcpyAsync(assign + C0, base + o_assign, (size_t)nc * 4, hipMemcpyDeviceToHost, L.stream));
        HIP_TRY(hipEventRecord(L.ev_done, L.stream));
        HIP_TRY(hipEventSynchronize(L.ev_done));
        finish_host_call(ctx, L);
        ms += g_last.ms;
        launches += g_last.launches;
        p0 = p1;
    }
    g_last.ms = ms;
    g_last.launches = launches;
    return LCSGPU_OK;
}

// CLARANS for many samples in one go: all sample triangles in one batched LCS launch, all float matrices in one launch,
// then ONE workgroup per sample runs that sample's whole chain of local searches (clarans_chain_kernel); the host only
// pre-draws the step positions and composes the shuffles (neither generator looks at a search, Clustering.cpp:43-46) --
// both depend on the shape (members, medoids) alone, so samples of one shape share them.
// The body of lcsgpu_clarans_batch and lcsgpu_clarans_large_batch.  allow_large: samples beyond the chain kernel's shapes
// (CLARANS_MAX_*) are not refused but run in clarans_large_chain_kernel, up to CLARANS_LARGE_MAX_MEMBERS members; the
// samples inside those shapes run through the chain kernel either way.
static int clarans_batch_impl(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* offsets, int32_t n_jobs, int distance_kind,
                              const int32_t* n_medoids, int32_t n_fixed, float explore_fraction, int32_t num_local, int32_t* medoids_out,
                              bool allow_large)
{
    if (!ctx) return fail(LCSGPU_E_INVALID, "NULL ctx");
    if (ctx->n < 0) return fail(LCSGPU_E_STATE, "no sequence set uploaded");
    if (!valid_kind(distance_kind)) return fail(LCSGPU_E_INVALID, "unknown distance kind %d", distance_kind);
    if (n_jobs < 0 || num_local < 1 || n_fixed < 0) return fail(LCSGPU_E_INVALID, "bad CLARANS batch");
    if (n_jobs == 0) return LCSGPU_OK;
    if (!ids || !offsets || !n_medoids || !medoids_out) return fail(LCSGPU_E_INVALID, "NULL argument");
    if (offsets[0] != 0) return fail(LCSGPU_E_INVALID, "offsets[0] must be 0");
    std::vector<int64_t> med_off((size_t)n_jobs + 1, 0);
    for (int32_t j = 0; j < n_jobs; ++j) {
        const int64_t n = offsets[j + 1] - offsets[j];
        const int32_t k = n_medoids[j];
        if (n < 1 || n > 0x7fffffff) return fail(LCSGPU_E_INVALID, "bad sample %d", j);
        if (k < 1 || k > n || n_fixed >= k)
            return fail(LCSGPU_E_INVALID, "bad CLARANS shape: %d medoids (%d fixed) of %lld, %d searches", k, n_fixed, (long long)n, num_local);
        if (allow_large) {
            if (n > lcsgpu::CLARANS_LARGE_MAX_MEMBERS)
                return fail(LCSGPU_E_UNSUPPORTED, "device CLARANS handles at most %d sample members (asked: %lld)", lcsgpu::CLARANS_LARGE_MAX_MEMBERS,
                            (long long)n);
        } else if (k > lcsgpu::CLARANS_MAX_MEDOIDS || n - k > lcsgpu::CLARANS_MAX_NONMEDOIDS)
            return fail(LCSGPU_E_UNSUPPORTED, "device CLARANS handles at most %d medoids and %d other sample members (asked: %d, %lld)",
                        lcsgpu::CLARANS_MAX_MEDOIDS, lcsgpu::CLARANS_MAX_NONMEDOIDS, k, (long long)(n - k));
        med_off[j + 1] = med_off[j] + k;
    }
    for (int64_t i = 0; i < offsets[n_jobs]; ++i)
        if (ids[i] < 0 || ids[i] >= ctx->n) return fail(LCSGPU_E_INVALID, "sample id %d out of range", ids[i]);

    // what depends on a sample's shape alone: the composed shuffles and the step positions
    struct Shape {
        int32_t n, k;
        std::vector<int32_t> perm; // [num_local][n]
        std::mt19937 gen_positions;
        std::vector<int32_t> draws;
        DevBuf d_perm, d_draws;
        int corrected = 0;
    };
    std::vector<std::unique_ptr<Shape>> shapes;
    struct Release {
        std::vector<std::unique_ptr<Shape>>& v;
        ~Release() { for (auto& s : v) { s->d_perm.release(); s->d_draws.release(); } }
    } release{shapes};
    std::vector<int> shape_of((size_t)n_jobs, -1);
    std::vector<int32_t> live; // the samples that need a search
    for (int32_t j = 0; j < n_jobs; ++j) {
        const int32_t n = (int32_t)(offsets[j + 1] - offsets[j]), k = n_medoids[j];
        int si = -1;
        for (size_t t = 0; t < shapes.size(); ++t)
            if (shapes[t]->n == n && shapes[t]->k == k) si = (int)t;
        if (si < 0) {
            shapes.emplace_back(new Shape);
            Shape& sh = *shapes.back();
            sh.n = n;
            sh.k = k;
            // Clustering.cpp:21-29: how many non-improving steps end a local search
            const int n_swaps = (n - k) * k, min_max_neighbor = 250;
            const int max_neighbor = n_swaps < min_max_neighbor ? n_swaps : std::max((int)(explore_fraction * n_swaps), min_max_neighbor);
            sh.corrected = max_neighbor / k;
            // partial_shuffle(candidate + n_fixed, candidate + n, candidate + n, gen_nodes) before every local search
            // (deterministic_random.h:113-127), applied to positions: where[i] = the position whose content ends up at i
            std::mt19937 gen_nodes;
            sh.perm.resize((size_t)num_local * n);
            std::vector<int32_t> where((size_t)n);
            for (int it = 0; it < num_local; ++it) {
                for (int32_t i = 0; i < n; ++i) where[(size_t)i] = i;
                int32_t* first = where.data() + n_fixed;
                const long cnt = n - n_fixed, N = cnt - 1;
                for (long i = 0; i < cnt; ++i) {
                    const unsigned long d = (unsigned long)N - (unsigned long)i + 1;
                    const unsigned long r = (unsigned long)gen_nodes(); // < 2^32: never in the rejected tail of a 64-bit range
                    std::swap(first[i], first[(r % d) + (unsigned long)i]);
                }
                std::copy(where.begin(), where.end(), sh.perm.begin() + (size_t)it * n);
            }
            si = (int)shapes.size() - 1;
        }
        shape_of[(size_t)j] = si;
        if (n == k) {
            // every member is a medoid: no step is ever drawn, every search costs 0, the first one stands
            // (Clustering.cpp:239-257: a later search has to be cheaper) -- its medoids are the order after the first shuffle
            std::copy(shapes[(size_t)si]->perm.begin(), shapes[(size_t)si]->perm.begin() + n, medoids_out + med_off[j]);
        } else
            live.push_back(j);
    }
    if (live.empty()) return LCSGPU_OK;

    const auto t_call = std::chrono::steady_clock::now();
    LaneGuard guard(ctx, LaneGuard::FRONT);
    Lane& L = guard.lane();
    HIP_TRY(hipSetDevice(ctx->device));
    const bool profile = getenv("LCSGPU_PROFILE") != nullptr;
    double t_prof[6] = {0};
    auto t_mark = std::chrono::steady_clock::now();
    auto lap = [&](int what, bool sync) {
        if (sync) (void)hipStreamSynchronize(L.stream);
        if (!profile) return;
        const auto t = std::chrono::steady_clock::now();
        t_prof[what] += std::chrono::duration<double>(t - t_mark).count();
        t_mark = t;
    };
    std::unique_lock<ComputeGate> wave(ctx->gate, std::defer_lock);
    const int elem = ctx->max_len > 65535 ? 4 : 2;
    std::vector<int64_t> tri_base;
    int64_t count = 0;
    bool had_long = false;
    int rc = batch_triangles_to_device(ctx, L, ids, offsets, n_jobs, elem, tri_base, &count, &had_long, [&] { lap(1, false); });
    if (rc) return rc;
    lap(2, profile);
    double lcs_ms = 0;
    int lcs_launches = 0;
    if (had_long) { // (synchronised list by list: the timing is in g_last)
        lcs_ms = g_last.ms;
        lcs_launches = g_last.launches;
    }
    // the samples' buffers, one allocation
    const int n_live = (int)live.size();
    const int64_t n_total = offsets[n_jobs];
    size_t at = 0;
    const size_t o_chains = at; at += a256((size_t)n_live * sizeof(lcsgpu::ClaransChain));
    const size_t o_states = at; at += a256((size_t)n_live * lcsgpu::CLARANS_STATE_WORDS * 4);
    const size_t o_ids = at; at += a256((size_t)n_total * 4);
    const size_t o_best = at; at += a256((size_t)med_off[n_jobs] * 4);
    struct Place { char* D; char* DM; char* cand; char* st; char* log; char* dn; };
    auto is_large = [&](int32_t j) { // beyond the chain kernel's registers: clarans_large_chain_kernel
        const int64_t n = offsets[j + 1] - offsets[j];
        return n_medoids[j] > lcsgpu::CLARANS_MAX_MEDOIDS || n - n_medoids[j] > lcsgpu::CLARANS_MAX_NONMEDOIDS;
    };
    std::vector<Place> place((size_t)n_live);
    int max_n = 0, max_k = 0;
    size_t sample_bytes = 0;
    {   // every sample's work area out of the context's chunks (this call owns them: it holds the FRONT lane); what the chunks
        // there are cannot hold comes out of ONE new chunk
        auto area = [&](int q, size_t* o_DM, size_t* o_cand, size_t* o_st, size_t* o_log, size_t* o_dn) {
            const int32_t j = live[(size_t)q];
            const size_t n = (size_t)(offsets[j + 1] - offsets[j]), k = (size_t)n_medoids[j];
            *o_DM = a256(n * n * 4);
            *o_cand = *o_DM + a256(n * k * 4);
            *o_st = *o_cand + a256(n * 4);
            *o_log = *o_st + a256(n * 16);
            *o_dn = *o_log + a256((n + 1) * 4);
            return *o_dn + (is_large(j) ? a256(n * 4) : 0);
        };
        size_t chunk = 0, used = 0; // the chunk being filled
        for (int q = 0; q < n_live; ++q) {
            const int32_t j = live[(size_t)q];
            const size_t n = (size_t)(offsets[j + 1] - offsets[j]), k = (size_t)n_medoids[j];
            size_t o_DM, o_cand, o_st, o_log, o_dn;
            const size_t o_D = 0, need = area(q, &o_DM, &o_cand, &o_st, &o_log, &o_dn);
            while (chunk < ctx->sample_chunks.size() && ctx->sample_chunks[chunk].cap - used < need) {
                ++chunk;
                used = 0;
            }
            if (chunk == ctx->sample_chunks.size()) {
                ctx->sample_chunks.emplace_back();
                size_t rest = 0, a, b, c, d, e;
                for (int r = q; r < n_live; ++r) rest += area(r, &a, &b, &c, &d, &e);
                rc = reserve_big(ctx, ctx->sample_chunks.back(), rest, "CLARANS samples");
                if (rc) {
                    ctx->sample_chunks.pop_back();
                    return rc;
                }
                used = 0;
            }
            char* b = (char*)ctx->sample_chunks[chunk].p + used;
            place[(size_t)q] = Place{b + o_D, b + o_DM, b + o_cand, b + o_st, b + o_log, b + o_dn};
            used += need;
            sample_bytes += need;
            max_n = std::max(max_n, (int)n);
            if (!is_large(j)) max_k = std::max(max_k, (int)k); // (the chain kernel's instantiation: by its own chains)
        }
    }
    rc = reserve_big(ctx, L.d_work, at, "CLARANS batch tables");
    if (rc) return rc;
    at += sample_bytes; // (the profile line's figure)
    lap(3, false);
    char* base = (char*)L.d_work.p;
    const size_t host_bytes = a256((size_t)n_live * sizeof(lcsgpu::ClaransChain)) + a256((size_t)n_live * lcsgpu::CLARANS_STATE_WORDS * 4);
    HIP_TRY(L.h_small.reserve(host_bytes));
    lcsgpu::ClaransChain* h_chains = (lcsgpu::ClaransChain*)L.h_small.p;
    int32_t* h_states = (int32_t*)((char*)L.h_small.p + a256((size_t)n_live * sizeof(lcsgpu::ClaransChain)));
    static const int draws_first = std::max(16, tune_int("clarans_draws", 65536)), slice_us = std::max(0, tune_int("clarans_slice_us", 0));
    // a launch of clarans_large_chain_kernel ends after that long and its chains go on in the next (0 = no limit): such a chain
    // can run for seconds, and no launch should
    static const int large_slice_us = std::max(0, tune_int("clarans_large_slice_us", 250000));
    for (auto& shp : shapes) {
        Shape& sh = *shp;
        if (sh.n == sh.k) continue;
        HIP_TRY(sh.d_perm.reserve(sh.perm.size() * 4));
        HIP_TRY(hipMemcpyAsync(sh.d_perm.p, sh.perm.data(), sh.perm.size() * 4, hipMemcpyHostToDevice, L.stream));
    }
    // det_uniform_int_distribution<int>(k, n - 1) over gen_positions (deterministic_random.h:62-76), `want` of them
    auto extend_draws = [&](Shape& sh, size_t want) -> int {
        if (sh.draws.size() >= want) return LCSGPU_OK;
        const uint32_t k = (uint32_t)sh.k, diff = (uint32_t)(sh.n - sh.k);
        const uint32_t bad = 0xffffffffu / diff;
        sh.draws.reserve(want);
        while (sh.draws.size() < want) {
            const uint32_t r = sh.gen_positions();
            if (r / diff < bad) sh.draws.push_back((int32_t)(r % diff + k));
        }
        HIP_TRY(sh.d_draws.reserve(want * 4)); // (only between launches: nothing reads the old array)
        HIP_TRY(hipMemcpyAsync(sh.d_draws.p, sh.draws.data(), sh.draws.size() * 4, hipMemcpyHostToDevice, L.stream));
        return LCSGPU_OK;
    };
    for (auto& shp : shapes)
        if (shp->n != shp->k) {
            rc = extend_draws(*shp, (size_t)draws_first);
            if (rc) return rc;
        }
    HIP_TRY(hipMemcpyAsync(base + o_ids, ids, (size_t)n_total * 4, hipMemcpyHostToDevice, L.stream));
    memset(h_states, 0, (size_t)n_live * lcsgpu::CLARANS_STATE_WORDS * 4);
    const float flt_max = std::numeric_limits<float>::max();
    for (int q = 0; q < n_live; ++q) {
        const int32_t j = live[(size_t)q];
        const Shape& sh = *shapes[(size_t)shape_of[(size_t)j]];
        lcsgpu::ClaransChain& c = h_chains[q];
        memset(&c, 0, sizeof c);
        const Place& p = place[(size_t)q];
        c.a.D = (const float*)p.D;
        c.a.DMt = (float*)p.DM;
        c.a.cand = (int32_t*)p.cand;
        c.a.st = (float4*)p.st;
        c.a.cost_log = (float*)p.log;
        c.a.state = (int32_t*)(base + o_states) + (size_t)q * lcsgpu::CLARANS_STATE_WORDS;
        c.a.n_elems = sh.n;
        c.a.n_medoids = sh.k;
        c.a.n_fixed = n_fixed;
        c.a.corrected = sh.corrected;
        c.a.draws = (const int32_t*)sh.d_draws.p;
        c.a.draws_len = (int32_t)sh.draws.size();
        c.perm = (const int32_t*)sh.d_perm.p;
        c.ids = (const int32_t*)(base + o_ids) + offsets[j];
        c.best = (int32_t*)(base + o_best) + med_off[j];
        c.tri0 = tri_base[(size_t)j];
        c.num_local = num_local;
        c.dn_member = is_large(j) ? (float*)p.dn : nullptr;
        int32_t* st = h_states + (size_t)q * lcsgpu::CLARANS_STATE_WORDS;
        st[4] = 1;  // ST_FRESH
        st[10] = 1; // ST_FIRST
        memcpy(&st[17], &flt_max, 4); // ST_BEST
        st[18] = 1; // ST_NEED_INIT
    }
    HIP_TRY(hipMemcpyAsync(base + o_states, h_states, (size_t)n_live * lcsgpu::CLARANS_STATE_WORDS * 4, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(hipMemcpyAsync(base + o_chains, h_chains, (size_t)n_live * sizeof(lcsgpu::ClaransChain), hipMemcpyHostToDevice, L.stream));
    HIP_TRY(lcsgpu::launch_subset_distances_batch(L.d_out.p, elem, (const lcsgpu::ClaransChain*)(base + o_chains), n_live, max_n,
                                                  (const uint32_t*)ctx->d_lens.p, (const float*)ctx->d_powf.p, distance_kind, L.stream));
    // the triangles and distances ran beside the other lanes' work (this lane's stream goes first); the chains run alone:
    // the chip to them (lcsgpu_internal.h, ComputeGate)
    HIP_TRY(hipEventRecord(L.ev_done, L.stream));
    HIP_TRY(hipEventSynchronize(L.ev_done));
    lap(4, false);
    wave.lock();
    lap(0, false);
    // the chains: normally one launch; a chain that runs out of positions (or, under LCSGPU_TUNE clarans_slice_us, of time)
    // comes back for another
    std::vector<int> todo;
    todo.reserve((size_t)n_live);
    int n_large = 0;
    for (int q = 0; q < n_live; ++q)
        if (!is_large(live[(size_t)q])) todo.push_back(q);
    for (int q = 0; q < n_live; ++q)
        if (is_large(live[(size_t)q])) {
            todo.push_back(q);
            ++n_large;
        }
    std::vector<lcsgpu::ClaransChain> all(h_chains, h_chains + n_live);
    int launches = 0, large_launches = 0;
    long accepts = 0, steps = 0;
    std::vector<int32_t> ticks, where;
    while (!todo.empty()) {
        const int nt = (int)todo.size();
        int nt_small = 0; // (todo keeps its order: the chain kernel's chains first)
        while (nt_small < nt && !is_large(live[(size_t)todo[(size_t)nt_small]])) ++nt_small;
        for (int t = 0; t < nt; ++t) {
            lcsgpu::ClaransChain& c = h_chains[t];
            c = all[(size_t)todo[(size_t)t]];
            const Shape& sh = *shapes[(size_t)shape_of[(size_t)live[(size_t)todo[(size_t)t]]]];
            c.a.draws = (const int32_t*)sh.d_draws.p;
            c.a.draws_len = (int32_t)sh.draws.size();
        }
        HIP_TRY(hipMemcpyAsync(base + o_chains, h_chains, (size_t)nt * sizeof(lcsgpu::ClaransChain), hipMemcpyHostToDevice, L.stream));
        HIP_TRY(lcsgpu::launch_clarans_chains((const lcsgpu::ClaransChain*)(base + o_chains), nt_small, max_k, slice_us, L.stream));
        HIP_TRY(lcsgpu::launch_clarans_large_chains((const lcsgpu::ClaransChain*)(base + o_chains) + nt_small, nt - nt_small, large_slice_us, L.stream));
        large_launches += nt > nt_small;
        HIP_TRY(hipMemcpyAsync(h_states, base + o_states, (size_t)n_live * lcsgpu::CLARANS_STATE_WORDS * 4, hipMemcpyDeviceToHost, L.stream));
        HIP_TRY(hipEventRecord(L.ev_done, L.stream));
        HIP_TRY(hipEventSynchronize(L.ev_done));
        L.plan_in_flight = false;
        ++launches;
        std::vector<int> again;
        // more pre-drawn positions: ONE target per shape and round, however many of its chains ran out -- twice what the
        // shape had when the round began, or what the chain that is furthest asks for
        std::vector<size_t> want(shapes.size(), 0);
        for (int q : todo) {
            const int32_t* st = h_states + (size_t)q * lcsgpu::CLARANS_STATE_WORDS;
            if (st[1]) { // ST_DONE: the whole chain
                accepts += st[3];
                steps += st[12];
                ticks.push_back(st[19]);
                where.push_back(st[20]);
                continue;
            }
            again.push_back(q);
            if (st[7]) { // ST_MORE_DRAWS
                const size_t si = (size_t)shape_of[(size_t)live[(size_t)q]];
                want[si] = std::max(want[si], std::max(shapes[si]->draws.size() * 2, (size_t)st[0] + (size_t)st[8] + (size_t)draws_first));
            }
        }
        for (size_t si = 0; si < shapes.size(); ++si)
            if (want[si]) {
                if (want[si] > 0x7fffffffu) return fail(LCSGPU_E_UNSUPPORTED, "a CLARANS chain needs more than 2^31 step positions");
                rc = extend_draws(*shapes[si], want[si]);
                if (rc) return rc;
            }
        todo.swap(again);
        if (launches > 100000) return fail(LCSGPU_E_STATE, "CLARANS batch does not finish");
    }
    // the results: live samples' medoids (the others were written above)
    std::vector<int32_t> best((size_t)med_off[n_jobs]);
    HIP_TRY(hipMemcpyAsync(best.data(), base + o_best, best.size() * 4, hipMemcpyDeviceToHost, L.stream));
    HIP_TRY(hipStreamSynchronize(L.stream));
    for (int32_t j : live) std::copy(best.begin() + med_off[j], best.begin() + med_off[j + 1], medoids_out + med_off[j]);
    if (!had_long) finish_host_call(ctx, L);
    else note_host_call(ctx, lcs_ms, lcs_launches);
    if (getenv("LCSGPU_PROFILE") && !ticks.empty()) {
        std::vector<int32_t> sorted(ticks);
        std::sort(sorted.begin(), sorted.end());
        std::map<int, int> per_cu;
        for (int32_t w : where) ++per_cu[w];
        int shared_cu = 0;
        for (auto& kv : per_cu) shared_cu += kv.second > 1 ? kv.second : 0;
        double slow_shared = 0, slow_alone = 0;
        int n_sh = 0, n_al = 0;
        for (size_t i = 0; i < ticks.size(); ++i) {
            if (per_cu[where[i]] > 1) { slow_shared += ticks[i]; ++n_sh; } else { slow_alone += ticks[i]; ++n_al; }
        }
        fprintf(stderr, "clarans.batch chains: run time min %.1f median %.1f max %.1f ms; %d of %zu shared a CU (mean %.1f ms against %.1f ms alone)\n",
                sorted.front() * 1e-5, sorted[sorted.size() / 2] * 1e-5, sorted.back() * 1e-5, shared_cu, ticks.size(),
                n_sh ? slow_shared / n_sh * 1e-5 : 0.0, n_al ? slow_alone / n_al * 1e-5 : 0.0);
    }
    lap(5, false);
    if (profile)
        fprintf(stderr, "clarans.batch parts: gate %.1f ms, planning the triangles %.1f, their kernels %.1f, work area (%.2f GB) %.1f, tables + distances %.1f, chains + results %.1f\n",
                1e3 * t_prof[0], 1e3 * t_prof[1], 1e3 * t_prof[2], at / 1e9, 1e3 * t_prof[3], 1e3 * t_prof[4], 1e3 * t_prof[5]);
    if (getenv("LCSGPU_PROFILE") && n_large)
        fprintf(stderr, "clarans.large: %d chain(s) beyond the chain kernel's shapes, %d launch(es) of at most %d us\n", n_large, large_launches, large_slice_us);
    if (getenv("LCSGPU_PROFILE"))
        fprintf(stderr, "clarans.batch: %d samples (%d searched, %zu shapes), %d launch(es), %ld accepts, %ld steps looked at, %.3f s\n", n_jobs, n_live,
                shapes.size(), launches, accepts, steps, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_call).count());
    return LCSGPU_OK;
}

extern "C" { // every call through `guarded`

int lcsgpu_lcs_triangles_batch(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups,
                               void* out, int elem_size)
{
    return guarded("lcs_triangles_batch", lcs_triangles_batch_impl, ctx, ids, group_offsets, n_groups, out, elem_size);
}

int lcsgpu_mst_prim_batch(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, int distance_kind,
                          lcsgpu_mst_edge* out_edges)
{
    return guarded("batched MST", mst_prim_batch_impl, ctx, ids, group_offsets, n_groups, distance_kind, out_edges);
}

int lcsgpu_upgma_batch(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, int distance_kind,
                       int modified, int32_t* out_left, int32_t* out_right, int32_t* out_status)
{
    return guarded("batched UPGMA", upgma_batch_impl, ctx, ids, group_offsets, n_groups, distance_kind, modified, out_left, out_right, out_status);
}

int lcsgpu_nj_batch(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* group_offsets, int32_t n_groups, int distance_kind,
                    int32_t* out_left, int32_t* out_right, int32_t* out_status)
{
    return guarded("batched NJ", nj_batch_impl, ctx, ids, group_offsets, n_groups, distance_kind, out_left, out_right, out_status);
}

int lcsgpu_dist_text_batch(lcsgpu_ctx* ctx, const char* names, const uint64_t* name_offsets, const int32_t* ids,
                           const int64_t* group_offsets, int32_t n_groups, int distance_kind, int flags, const char** text,
                           uint64_t* text_offsets)
{
    return guarded("batched text", dist_text_batch_impl, ctx, names, name_offsets, ids, group_offsets, n_groups, distance_kind, flags, text, text_offsets);
}

int lcsgpu_assign_seeds(lcsgpu_ctx* ctx, const int32_t* seed_ids, int32_t n_seeds, const int32_t* col_ids,
                        int32_t n_cols, int distance_kind, int32_t first_k, float* dist, int32_t* assign)
{
    return guarded("assign_seeds", assign_seeds_impl, ctx, seed_ids, n_seeds, col_ids, n_cols, distance_kind, first_k, dist, assign);
}

int lcsgpu_assign_seeds_batch(lcsgpu_ctx* ctx, const int32_t* seed_ids, const int64_t* seed_offsets, const int32_t* col_ids,
                              const int64_t* col_offsets, int32_t n_jobs, int distance_kind, float* dist, int32_t* assign)
{
    return guarded("assign_seeds_batch", assign_seeds_batch_impl, ctx, seed_ids, seed_offsets, col_ids, col_offsets, n_jobs, distance_kind, dist, assign);
}

int lcsgpu_clarans_batch(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* offsets, int32_t n_jobs, int distance_kind,
                         const int32_t* n_medoids, int32_t n_fixed, float explore_fraction, int32_t num_local, int32_t* medoids_out)
{
    return guarded("CLARANS batch", clarans_batch_impl, ctx, ids, offsets, n_jobs, distance_kind, n_medoids, n_fixed, explore_fraction, num_local, medoids_out, false);
}

int lcsgpu_clarans_large_batch(lcsgpu_ctx* ctx, const int32_t* ids, const int64_t* offsets, int32_t n_jobs, int distance_kind,
                               const int32_t* n_medoids, int32_t n_fixed, float explore_fraction, int32_t num_local, int32_t* medoids_out)
{
    return guarded("CLARANS batch", clarans_batch_impl, ctx, ids, offsets, n_jobs, distance_kind, n_medoids, n_fixed, explore_fraction, num_local, medoids_out, true);
}

int lcsgpu_clarans(lcsgpu_ctx* ctx, const int32_t* ids, int32_t n_ids, int distance_kind, int32_t n_medoids,
                   int32_t n_fixed, float explore_fraction, int32_t num_local, int32_t* medoids_out)
{
    if (!ids || !medoids_out || n_ids < 1) return fail(LCSGPU_E_INVALID, "bad sample / output");
    const int64_t offsets[2] = {0, n_ids};
    return lcsgpu_clarans_batch(ctx, ids, offsets, 1, distance_kind, &n_medoids, n_fixed, explore_fraction, num_local, medoids_out);
}

int lcsgpu_clarans_large(lcsgpu_ctx* ctx, const int32_t* ids, int32_t n_ids, int distance_kind, int32_t n_medoids,
                         int32_t n_fixed, float explore_fraction, int32_t num_local, int32_t* medoids_out)
{
    if (!ids || !medoids_out || n_ids < 1) return fail(LCSGPU_E_INVALID, "bad sample / output");
    const int64_t offsets[2] = {0, n_ids};
    return lcsgpu_clarans_large_batch(ctx, ids, offsets, 1, distance_kind, &n_medoids, n_fixed, explore_fraction, num_local, medoids_out);
}

} // extern "C"
