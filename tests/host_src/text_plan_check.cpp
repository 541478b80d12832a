// text_plan_check.cpp -- the tables of the batched text launches (famsa_amd/csrc/text_plan.h), checked without a GPU: the
// plan of a call is replayed the way the kernels walk it (text_kernels.hip: workgroup b = job b, its row job_row[b], its
// segment b - job0, thread t's slot s = value seg * TEXT_SEG + t * TEXT_PER_THREAD + s) and
//   every (list, row, column) value is owned by exactly one (job, thread, slot),
//   every source index lies inside its own list's triangle or rectangle, at the place the LCS launches write it,
//   every row -- one without values too: its "name\n" -- has a first segment, and a row's jobs are consecutive,
//   the lists' first rows and sources are the prefixes the host layer slices the text by.
// Lists of 0, 1, 2, 1023, 1024, 1025, 2049 and a few random sizes, alone and mixed in one call, lower and square form.
// Prints "ok ..." and exits 0, or says what is wrong and exits 1.  Built by famsa_amd/csrc/Makefile with the host compiler;
// tests/test_text_plan.py runs it.
#include "../../famsa_amd/csrc/text_plan.h"

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
static char g_where[160];

static long long g_values = 0, g_jobs = 0, g_rows = 0;

static void check_call(const std::vector<int64_t>& sizes, bool square, const char* name)
{
    snprintf(g_where, sizeof g_where, "%s, %s form, %zu lists", name, square ? "square" : "lower", sizes.size());
    std::vector<int64_t> offs(1, 0);
    for (int64_t m : sizes) offs.push_back(offs.back() + m);
    const int32_t G = (int32_t)sizes.size();
    TextPlan p;
    CHECK(plan_text(offs.data(), G, square, p), "the plan was refused");
    const int64_t n_rows = offs.back(), n_jobs = (int64_t)p.job_row.size();
    CHECK((int64_t)p.rows.size() == n_rows + 1, "%zu row records for %lld rows", p.rows.size(), (long long)n_rows);
    CHECK((int64_t)p.list_row0.size() == G + 1 && (int64_t)p.list_src0.size() == G + 1, "list tables");
    CHECK(p.rows[(size_t)n_rows].job0 == n_jobs, "the sentinel row's job0 is %d, jobs: %lld", p.rows[(size_t)n_rows].job0, (long long)n_jobs);
    // the lists: rows and sources are prefixes
    int64_t src = 0;
    for (int32_t g = 0; g <= G; ++g) {
        CHECK(p.list_row0[(size_t)g] == offs[(size_t)g], "list %d starts at row %lld", g, (long long)p.list_row0[(size_t)g]);
        CHECK(p.list_src0[(size_t)g] == src, "list %d's values start at %lld, want %lld", g, (long long)p.list_src0[(size_t)g], (long long)src);
        if (g < G) src += square ? sizes[(size_t)g] * sizes[(size_t)g] : sizes[(size_t)g] * (sizes[(size_t)g] - 1) / 2;
    }
    // the rows: what the kernels take from a record
    std::vector<int32_t> list_of((size_t)n_rows);
    for (int32_t g = 0; g < G; ++g)
        for (int64_t r = offs[(size_t)g]; r < offs[(size_t)g + 1]; ++r) list_of[(size_t)r] = g;
    for (int64_t r = 0; r < n_rows; ++r) {
        const TextRow& R = p.rows[(size_t)r];
        const int32_t g = list_of[(size_t)r];
        const int64_t m = sizes[(size_t)g], k = r - offs[(size_t)g];
        CHECK(R.pos == r && R.pos0 == offs[(size_t)g], "row %lld: member position %d of the list at %d", (long long)r, R.pos, R.pos0);
        CHECK(R.cols == (square ? m : k), "row %lld has %d columns", (long long)r, R.cols);
        CHECK(R.src == p.list_src0[(size_t)g] + (square ? k * m : k * (k - 1) / 2), "row %lld: source %lld", (long long)r, (long long)R.src);
        const int32_t segs = p.rows[(size_t)r + 1].job0 - R.job0;
        CHECK(segs >= 1, "row %lld has no job: its name would not be written", (long long)r);
        CHECK(segs == (R.cols > 0 ? (R.cols + TEXT_SEG - 1) / TEXT_SEG : 1), "row %lld: %d segments for %d columns", (long long)r, segs, R.cols);
        // (columns are read as members pos0 + c: inside the list)
        CHECK(R.cols <= m, "row %lld reads %d members of a list of %lld", (long long)r, R.cols, (long long)m);
    }
    // the jobs: replayed as the kernels walk them
    std::vector<uint8_t> owned((size_t)p.list_src0[(size_t)G], 0);
    std::vector<int32_t> row_values((size_t)n_rows, 0);
    for (int64_t b = 0; b < n_jobs; ++b) {
        const int32_t r = p.job_row[(size_t)b];
        CHECK(r >= 0 && r < n_rows, "job %lld names row %d", (long long)b, r);
        const TextRow& R = p.rows[(size_t)r];
        const int32_t seg = (int32_t)(b - R.job0);
        CHECK(seg >= 0 && b < p.rows[(size_t)r + 1].job0, "job %lld is not among the jobs of its row %d", (long long)b, r);
        const int32_t g = list_of[(size_t)r];
        for (int t = 0; t < TEXT_THREADS; ++t)
            for (int s = 0; s < TEXT_PER_THREAD; ++s) {
                const int64_t j = (int64_t)seg * TEXT_SEG + t * TEXT_PER_THREAD + s;
                if (j >= R.cols) continue;
                const int64_t at = R.src + j;
                CHECK(at >= p.list_src0[(size_t)g] && at < p.list_src0[(size_t)g + 1], "row %d column %lld reads %lld, outside list %d", r, (long long)j,
                      (long long)at, g);
                CHECK(!owned[(size_t)at], "row %d column %lld: a second owner", r, (long long)j);
                owned[(size_t)at] = 1;
                ++row_values[(size_t)r];
                ++g_values;
            }
        if (R.cols > 0) CHECK((int64_t)seg * TEXT_SEG < R.cols, "job %lld: segment %d of row %d is empty", (long long)b, seg, r);
    }
    for (int64_t r = 0; r < n_rows; ++r)
        CHECK(row_values[(size_t)r] == p.rows[(size_t)r].cols, "row %lld: %d of %d values owned", (long long)r, row_values[(size_t)r], p.rows[(size_t)r].cols);
    // lower form: the triangle holds exactly the rows' values; square form: the rectangle does
    for (size_t at = 0; at < owned.size(); ++at) CHECK(owned[at], "value %zu of the call has no owner", at);
    g_jobs += n_jobs;
    g_rows += n_rows;
}

int main()
{
    static const int64_t SIZES[] = {0, 1, 2, 1023, 1024, 1025, 2049};
    std::mt19937 gen(20260);
    int calls = 0;
    for (int square = 0; square < 2; ++square) {
        check_call({}, square != 0, "no list");
        ++calls;
        for (int64_t m : SIZES) { // alone
            char name[64];
            snprintf(name, sizeof name, "one list of %lld", (long long)m);
            check_call({m}, square != 0, name);
            ++calls;
        }
        check_call(std::vector<int64_t>(SIZES, SIZES + 7), square != 0, "the seam sizes in one call");
        check_call({2049, 0, 1, 1025, 0, 2, 1024, 1, 1023, 0}, square != 0, "the seam sizes shuffled, empty lists between");
        std::vector<int64_t> many;
        for (int i = 0; i < 300; ++i) many.push_back((int64_t)(gen() % 120));
        many.push_back(1500 + (int64_t)(gen() % 1000));
        for (int i = 0; i < 40; ++i) many.push_back((int64_t)(gen() % 400));
        check_call(many, square != 0, "random sizes");
        calls += 3;
    }
    printf("ok: %d calls, %lld rows, %lld jobs, %lld values owned once\n", calls, g_rows, g_jobs, g_values);
    return 0;
}
