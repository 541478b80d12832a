// job_plan.h -- the job tables of the batched LCS launches (lcsgpu_lcs_triangles_batch and what builds on it,
// lcsgpu_assign_seeds_batch) as plain host code: which refs share a launch, which refs and columns a workgroup gets.
// No HIP and no lcsgpu_ctx in here, so that tests/host_src/job_plan_check.cpp can replay a plan cell by cell without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lcsgpu_impl {

// Which instantiation the refs of every half-word class run in.  A call's classes are launches one after the other on
// one stream, and a launch that cannot fill the chip lasts as long as one of its workgroups however few it has: the
// sample triangle of a FastTree split (2000 family members, four classes of ~500 refs, ~500 workgroups each) took four
// times ~160 us (profiles/clarans_rounds_r04.txt: 4373 such launches, 1.22 s of kernel time for work that fills the chip
// for 0.3 s).  So neighbouring classes are run together in the larger one's kernel -- a ref's half-words beyond its own
// are all-ones no-ops (h_class) -- as long as the group stays below the workgroup count a launch is planned for
// (refs_per_block_for: 2048).  wgs[h] = workgroups class h would have with the fewest refs per workgroup, h = 1 .. 64;
// target[h] >= h.  Classes that fill the chip on their own (every large triangle) are left alone, as are the
// orientation-sensitive and long refs.
inline void merge_small_classes(const double* wgs, int* target)
{
    const double want = 2048.0;
    for (int h = 0; h <= 64; ++h) target[h] = h;
    int first = -1; // first class of the open group
    double sum = 0;
    auto close = [&](int last) {
        if (first > 0)
            for (int h = first; h <= last; ++h)
                if (wgs[h] > 0) target[h] = last;
        first = -1;
        sum = 0;
    };
    int last_used = -1;
    for (int h = 1; h <= 64; ++h) {
        if (wgs[h] <= 0) continue;
        if (first > 0 && sum + wgs[h] > want) close(last_used);
        if (wgs[h] >= want) { // fills the chip by itself
            close(last_used);
            last_used = h;
            continue;
        }
        if (first < 0) first = h;
        sum += wgs[h];
        last_used = h;
    }
    close(last_used);
}

// What a workgroup of a job-table launch does: refs [k0, k0 + nk) of its bucket against the columns [c0, limit) of its
// block (RowsArgs::jobs: the int4 the kernel reads).
struct Job { int32_t k0, nk, c0, limit; };

// A ref as its caller hands it to plan_jobs.  A unit is what a workgroup never crosses: an id list (triangles) or a
// piece (rectangles); columns are positions in the launch's concatenated column list.
struct JobRef {
    int32_t id, unit;
    int32_t col0;    // the unit's first column
    int64_t col_end; // triangles: the ref's own row, where its columns end; rectangles: the end of the piece
    int64_t out0;    // where the unit's triangle, or the ref's row of the rectangle, starts in the output
    double weight;   // the workgroups it adds to its class for merge_small_classes (a plain ref's)
    uint8_t cls;     // lcsgpu_ctx::ref_class: the half-word class | 0x80 for an orientation-sensitive ref ...
    uint8_t quirk_bv; // ... whose kernel is quirk_h_class of its length
    bool narrow;     // one-wave workgroups, column blocks of 64 (RowsArgs::block_threads)
};

// per instantiated kernel: its refs (in the caller's order, so the refs of one unit are adjacent) and its jobs
struct JobBucket {
    int bv;
    bool quirk, narrow;
    std::vector<JobRef> refs; // (col_end in triangle mode = RowsArgs::ref_rows)
    std::vector<Job> jobs;
    int refs_per_wg = 0;
};

using RefsPerWg = int (*)(int h, bool quirk, long n_refs, long col_blocks, bool fused); // lcsgpu::refs_per_block_for

// The refs split by instantiated kernel -- the half-word class after merge_small_classes, the quirk flag, the workgroup
// width -- and every bucket cut into jobs of at most R refs of one unit times one column block, up to the last ref's
// column end.  col_blocks: what R is asked with.  false: a bucket has more jobs than a grid takes.
inline bool plan_jobs(const std::vector<JobRef>& refs, long col_blocks, RefsPerWg refs_per_wg, std::vector<JobBucket>& buckets)
{
    double wgs[65] = {0};
    for (const JobRef& r : refs)
        if (!(r.cls & 0x80)) wgs[r.cls] += r.weight;
    int target[65];
    merge_small_classes(wgs, target);
    int index_of[320];
    std::fill(index_of, index_of + 320, -1);
    buckets.clear();
    for (const JobRef& r : refs) {
        const bool q = (r.cls & 0x80) != 0;
        const int bv = q ? r.quirk_bv : target[r.cls];
        const int key = bv * 2 + (q ? 1 : 0) + (r.narrow ? 160 : 0);
        if (index_of[key] < 0) {
            index_of[key] = (int)buckets.size();
            buckets.push_back(JobBucket{bv, q, r.narrow, {}, {}, 0});
            // (hundreds of lists: growing this step by step was a third of the planning time)
            buckets.back().refs.reserve(refs.size() / (buckets.size() > 1 ? 4 : 1) + 16);
        }
        buckets[index_of[key]].refs.push_back(r);
    }
    for (JobBucket& b : buckets) {
        const size_t nr = b.refs.size();
        const size_t R = (size_t)std::max(1, b.refs_per_wg = refs_per_wg(b.bv, b.quirk, (long)nr, col_blocks, false));
        b.jobs.reserve(nr / R * (b.narrow ? 3 : 5) + 16);
        for (size_t k0 = 0, k1; k0 < nr; k0 = k1) {
            for (k1 = k0 + 1; k1 < nr && k1 - k0 < R && b.refs[k1].unit == b.refs[k0].unit;) ++k1;
            const int64_t limit = b.refs[k1 - 1].col_end; // (column ends ascend inside a unit)
            for (int64_t c0 = b.refs[k0].col0; c0 < limit; c0 += b.narrow ? 64 : 256)
                b.jobs.push_back(Job{(int32_t)k0, (int32_t)(k1 - k0), (int32_t)c0, (int32_t)limit});
        }
        if (b.jobs.size() > 0x7fffffffu) return false;
    }
    return true;
}

} // namespace lcsgpu_impl
