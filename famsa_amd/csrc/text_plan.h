// text_plan.h -- the tables of the batched text launches (lcsgpu_dist_text_batch, text_kernels.hip) as plain host code:
// lists -> rows -> (row, segment) jobs, every row's place in its list's packed triangle or m x m rectangle, its column count.
// No HIP and no lcsgpu_ctx in here, so that tests/host_src/text_plan_check.cpp can replay a plan value by value without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lcsgpu_impl {

// A text workgroup: TEXT_THREADS threads x TEXT_PER_THREAD consecutive values each = one segment of a row.  The kernels
// (text_kernels.hip) and the replay take the shape from here.
constexpr int TEXT_THREADS = 256;
constexpr int TEXT_PER_THREAD = 4;
constexpr int TEXT_SEG = TEXT_THREADS * TEXT_PER_THREAD;

// A row of the call: member `pos` (a position in the call's concatenated id list) of the list that starts at position pos0.
// Its value c is the 16-bit LCS at src + c, c < cols: src = the list's triangle + k (k - 1) / 2 in the lower form (cols = k,
// the row's number in its list), the list's rectangle + k m in the square form (cols = m).  Its segments are the jobs
// [job0, next row's job0): at least one, so that a row without values still writes "name\n".
struct TextRow {
    int64_t src;
    int32_t pos, pos0, cols, job0;
};

struct TextPlan {
    std::vector<TextRow> rows;        // n_rows + 1: the last entry carries job0 = the number of jobs (and src = all values)
    std::vector<int32_t> job_row;     // per job (= workgroup): its row; its segment = job - rows[row].job0
    std::vector<int64_t> list_row0;   // n_groups + 1: the first row of every list
    std::vector<int64_t> list_src0;   // n_groups + 1: where every list's triangle / rectangle starts; [n_groups] = all values
};

// A per-row table and a per-job row number, not a search: a workgroup gets its row with one 4-byte and one 24-byte load
// that every lane shares, where a binary search over the lists' row prefix costs log2(lists) dependent loads per workgroup
// and the row's place in its triangle a division on top; the tables are 28 B per row against ~9 B of text per VALUE.
// false: more rows or jobs than a 1-D grid and the 32-bit tables take.
inline bool plan_text(const int64_t* group_offsets, int32_t n_groups, bool square, TextPlan& p)
{
    p.rows.clear();
    p.job_row.clear();
    p.list_row0.assign((size_t)n_groups + 1, 0);
    p.list_src0.assign((size_t)n_groups + 1, 0);
    const int64_t n_rows = n_groups > 0 ? group_offsets[n_groups] - group_offsets[0] : 0;
    if (n_rows < 0 || n_rows > 0x7fffff00) return false;
    p.rows.reserve((size_t)n_rows + 1);
    p.job_row.reserve((size_t)n_rows + 16);
    int64_t src = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        const int64_t g0 = group_offsets[g], m = group_offsets[g + 1] - g0;
        p.list_row0[(size_t)g] = (int64_t)p.rows.size();
        p.list_src0[(size_t)g] = src;
        for (int64_t k = 0; k < m; ++k) {
            const int64_t cols = square ? m : k;
            const int64_t segs = cols > 0 ? (cols + TEXT_SEG - 1) / TEXT_SEG : 1;
            if ((int64_t)p.job_row.size() + segs > 0x7fffff00) return false;
            p.rows.push_back(TextRow{src + (square ? k * m : k * (k - 1) / 2), (int32_t)(g0 + k), (int32_t)g0, (int32_t)cols,
                                     (int32_t)p.job_row.size()});
            for (int64_t s = 0; s < segs; ++s) p.job_row.push_back((int32_t)(p.rows.size() - 1));
        }
        src += square ? m * m : m * (m - 1) / 2;
    }
    p.list_row0[(size_t)n_groups] = (int64_t)p.rows.size();
    p.list_src0[(size_t)n_groups] = src;
    p.rows.push_back(TextRow{src, 0, 0, 0, (int32_t)p.job_row.size()});
    return true;
}

} // namespace lcsgpu_impl
