// job_plan_check.cpp -- the job tables of the batched LCS launches (famsa_amd/csrc/job_plan.h), checked without a GPU:
// every wanted ref in one bucket of the right kernel, every bucket's jobs a partition of its refs that tiles their
// columns, and -- replaying the kernel's index formula (lcs_kernels.hip, store_result) over every (job, ref, column) --
// every cell of the output written exactly once.  Triangles (lcsgpu_lcs_triangles_batch) and rectangles
// (lcsgpu_assign_seeds_batch), four class mixes, three refs-per-workgroup policies.  Prints "ok ..." and exits 0, or says
// what is wrong and exits 1.  Built by famsa_amd/csrc/Makefile with the host compiler; tests/test_job_plan.py runs it.
#include "../../famsa_amd/csrc/job_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace lcsgpu_impl;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "%s [%s]: ", g_where, #cond);     \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)
static char g_where[128];

// ---- the three policies for R, in refs_per_block_for's shape ----
static int rg_of(int h, bool quirk) { return quirk ? 1 : h <= 16 ? 4 : h <= 32 ? 2 : 1; }
static int full_of(int h, bool quirk) // the full complement: tests/test_gpu_lcs_plans.py, FULL
{
    if (quirk) return h == 8 ? 32 : h == 16 ? 16 : h == 32 ? 8 : 4;
    static const int upto[] = {8, 10, 12, 16, 18, 20, 24, 32, 36, 42, 50, 64}, r[] = {32, 24, 20, 16, 14, 12, 10, 8, 7, 6, 5, 4};
    for (int i = 0;; ++i)
        if (h <= upto[i]) return r[i];
}
static int r_one(int, bool, long, long, bool) { return 1; }
static int r_group(int h, bool quirk, long, long, bool) { return rg_of(h, quirk); }
static int r_full(int h, bool quirk, long, long, bool) { return full_of(h, quirk); }
static const RefsPerWg POLICY[3] = {r_one, r_group, r_full};
static const char* const POLICY_NAME[3] = {"R=1", "R=register group", "R=full"};

static int quirk_class(int h) { return h <= 8 ? 8 : h <= 16 ? 16 : h <= 32 ? 32 : 64; } // lcs_kernels.hip, quirk_h_class

// ---- the class byte of a ref, by mix ----
enum { ONE_CLASS, SMALL_NEIGHBOURS, HEAVY_CLASS, QUIRKS, N_MIXES };
static const char* const MIX_NAME[N_MIXES] = {"one class", "small neighbours", "a heavy class", "quirk refs"};
static uint8_t draw_class(int mix, std::mt19937& gen)
{
    const unsigned u = gen() % 100;
    switch (mix) {
    case ONE_CLASS: return 10;
    case SMALL_NEIGHBOURS: return (uint8_t)(u < 25 ? 5 : u < 50 ? 6 : u < 75 ? 7 : 9);
    case HEAVY_CLASS: return (uint8_t)(u < 5 ? 18 : u < 10 ? 19 : u < 95 ? 20 : 21);
    default: { // a quarter of the refs orientation sensitive, the four quirk kernels alike
        static const int qh[4] = {3, 12, 25, 40};
        return (uint8_t)(u < 25 ? 0x80 | qh[u % 4] : 10);
    }
    }
}

static const int SIZES[] = {0, 1, 2, 63, 64, 65, 192, 193, 256, 257, 600}; // 192: the narrow limit
static const int NARROW_MAX = 192;

static long g_cells = 0, g_jobs = 0;

static void run(bool triangle, int mix, int policy)
{
    snprintf(g_where, sizeof g_where, "%s, %s, %s", triangle ? "triangles" : "rectangles", MIX_NAME[mix], POLICY_NAME[policy]);
    std::mt19937 gen(20240607u + (unsigned)(triangle * 100 + mix * 10 + policy));
    const RefsPerWg R_of = POLICY[policy];
    // the units: every size three times, in a drawn order
    std::vector<int> sizes;
    for (int rep = 0; rep < 3; ++rep)
        for (int s : SIZES) sizes.push_back(s);
    for (size_t i = sizes.size(); i > 1; --i) std::swap(sizes[i - 1], sizes[gen() % i]);
    // the refs as the two callers make them; a ref's id is its index in `refs` (the planner does not look at ids)
    std::vector<JobRef> refs;
    int64_t col = 0, count = 0;
    double wgs[65] = {0};
    for (size_t u = 0; u < sizes.size(); ++u) {
        const int64_t size = sizes[u], col0 = col;
        const int n_refs = triangle ? (int)std::max<int64_t>(0, size - 1) : 1 + (int)(gen() % 150);
        for (int r = 0; r < n_refs; ++r) {
            const uint8_t c = draw_class(mix, gen);
            const bool q = (c & 0x80) != 0;
            JobRef ref{};
            ref.id = (int32_t)refs.size();
            ref.unit = (int32_t)u;
            ref.col0 = (int32_t)col0;
            ref.col_end = triangle ? col0 + 1 + r : col0 + size; // the member's position (its row) | the piece's end
            ref.out0 = triangle ? count : count + (int64_t)r * size;
            const int64_t blocks = ((triangle ? 1 + r : size) + 255) / 256;
            ref.weight = q ? 0.0 : (double)blocks / R_of(c, false, 1, 1, false);
            ref.cls = c;
            ref.quirk_bv = (uint8_t)(q ? quirk_class(c & 0x7f) : 0);
            ref.narrow = triangle && !q && size <= NARROW_MAX;
            if (!q) wgs[c] += ref.weight;
            refs.push_back(ref);
        }
        col += size;
        count += triangle ? size * (size - 1) / 2 : (int64_t)n_refs * size;
    }
    const long col_blocks = triangle ? 1 : (long)std::max<int64_t>(1, col / 256 / (int64_t)sizes.size());
    std::vector<JobBucket> buckets;
    CHECK(plan_jobs(refs, col_blocks, R_of, buckets), "plan_jobs refused");

    // ---- refs ----
    std::vector<int> seen(refs.size(), 0);
    for (const JobBucket& b : buckets) {
        const size_t nr = b.refs.size();
        CHECK(nr > 0, "an empty bucket");
        CHECK(b.refs_per_wg == R_of(b.bv, b.quirk, (long)nr, col_blocks, false), "bucket h=%d: R=%d", b.bv, b.refs_per_wg);
        for (size_t k = 0; k < nr; ++k) {
            CHECK(b.refs[k].id >= 0 && (size_t)b.refs[k].id < refs.size(), "ref id %d", b.refs[k].id);
            CHECK(k == 0 || b.refs[k].id > b.refs[k - 1].id, "bucket h=%d: refs out of order at %zu", b.bv, k);
            const JobRef& r = refs[(size_t)b.refs[k].id];
            ++seen[(size_t)r.id];
            const bool q = (r.cls & 0x80) != 0;
            CHECK(b.quirk == q, "ref %d: quirk flag", r.id);
            if (q) CHECK(b.bv == quirk_class(r.cls & 0x7f), "quirk ref %d of class %d in h=%d", r.id, r.cls & 0x7f, b.bv);
            else CHECK(b.bv >= r.cls && b.bv <= 64, "ref %d of class %d in h=%d", r.id, r.cls, b.bv);
            CHECK(b.narrow == (triangle && !q && sizes[(size_t)r.unit] <= NARROW_MAX), "ref %d: narrow=%d", r.id, (int)b.narrow);
            CHECK(b.refs[k].unit == r.unit && b.refs[k].col0 == r.col0 && b.refs[k].col_end == r.col_end && b.refs[k].out0 == r.out0, "ref %d: its tables", r.id);
            // what the mixes are for
            if (mix == ONE_CLASS) CHECK(b.bv == 10, "one class, h=%d", b.bv);
            if (mix == SMALL_NEIGHBOURS && policy == 2) // (at most 3 / 32 of a workgroup per ref, 5400 refs at the most: one group)
                CHECK(b.bv == 9, "small neighbouring classes did not merge: class %d in h=%d", r.cls, b.bv);
            if (mix == HEAVY_CLASS && policy == 0) { // 18 and 19 share a launch, 20 fills the chip, 21 is on its own
                CHECK(wgs[20] >= 2048 && wgs[18] + wgs[19] < 2048 && wgs[21] < 2048, "the mix is not what it is meant to be");
                CHECK(b.bv == (r.cls == 18 ? 19 : r.cls), "a heavy class: class %d in h=%d", r.cls, b.bv);
            }
        }
    }
    for (size_t i = 0; i < refs.size(); ++i) CHECK(seen[i] == 1, "ref %zu is in %d buckets", i, seen[i]);

    // ---- jobs and cells ----
    std::vector<uint8_t> hit((size_t)count, 0);
    for (const JobBucket& b : buckets) {
        const size_t nr = b.refs.size(), nj = b.jobs.size();
        const int step = b.narrow ? 64 : 256;
        size_t j = 0;
        for (size_t k = 0; k < nr;) {
            if (j == nj || (size_t)b.jobs[j].k0 != k) { // no job starts here: the ref has no columns
                CHECK(b.refs[k].col_end <= b.refs[k].col0, "bucket h=%d: ref %zu has columns but no job", b.bv, k);
                ++k;
                continue;
            }
            const Job first = b.jobs[j];
            CHECK(first.nk >= 1 && first.nk <= b.refs_per_wg && k + (size_t)first.nk <= nr, "job %zu: %d refs, R=%d", j, first.nk, b.refs_per_wg);
            for (int r = 1; r < first.nk; ++r) CHECK(b.refs[k + r].unit == b.refs[k].unit, "job %zu crosses a unit", j);
            CHECK(first.limit == b.refs[k + first.nk - 1].col_end, "job %zu: limit %d", j, first.limit);
            // the run's column blocks tile [the unit's first column, limit)
            int64_t want_c0 = b.refs[k].col0;
            CHECK(want_c0 < first.limit, "job %zu has no column", j);
            for (; want_c0 < first.limit; want_c0 += step, ++j) {
                CHECK(j < nj, "bucket h=%d: jobs end before the columns of ref %zu", b.bv, k);
                const Job job = b.jobs[j];
                CHECK(job.k0 == first.k0 && job.nk == first.nk && job.limit == first.limit && job.c0 == want_c0,
                      "job %zu = {%d, %d, %d, %d}, expected column %lld of the run of ref %zu", j, job.k0, job.nk, job.c0, job.limit, (long long)want_c0, k);
                ++g_jobs;
                for (int r = 0; r < job.nk; ++r) { // store_result, batched rectangles | batched triangles
                    const size_t kk = k + (size_t)r;
                    for (int64_t c = job.c0; c < job.c0 + step && c < job.limit; ++c) {
                        int64_t idx;
                        if (!triangle)
                            idx = b.refs[kk].out0 + (c - b.refs[kk].col0);
                        else {
                            const int64_t row = b.refs[kk].col_end, g0 = b.refs[kk].col0, lr = row - g0;
                            if (c >= row) continue;
                            idx = b.refs[kk].out0 + lr * (lr - 1) / 2 + (c - g0);
                        }
                        CHECK(idx >= 0 && idx < count, "job %zu writes cell %lld of %lld", j, (long long)idx, (long long)count);
                        CHECK(!hit[(size_t)idx], "job %zu writes cell %lld again", j, (long long)idx);
                        hit[(size_t)idx] = 1;
                        ++g_cells;
                    }
                }
            }
            k += (size_t)first.nk;
        }
        CHECK(j == nj, "bucket h=%d: %zu jobs beyond its refs", b.bv, nj - j);
    }
    for (int64_t i = 0; i < count; ++i) CHECK(hit[(size_t)i], "cell %lld of %lld is never written", (long long)i, (long long)count);
}

int main()
{
    for (int triangle = 0; triangle < 2; ++triangle)
        for (int mix = 0; mix < N_MIXES; ++mix)
            for (int policy = 0; policy < 3; ++policy) run(triangle != 0, mix, policy);
    printf("ok: %d plans, %ld jobs, %ld cells, each written once\n", 2 * N_MIXES * 3, g_jobs, g_cells);
    return 0;
}
