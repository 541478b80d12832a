// text_kernels.hip -- the rows of -dist_export as TEXT, made on the device (gfx950).
//
// What the reference does per row on the host (tree/DistanceCalculator.cpp:88-113): "<id>," then every value through
// NumericConversions::Double2PChar(v, 6) (utils/conversion.h:109-119) separated by ',', the last separator replaced by
// '\n'.  Values are floats: (float) Transform<double, kind>(lcs, len_i, len_j) resp. Transform<float, pairwise_identity>
// (DistanceCalculator.cpp:36-76, tree/AbstractTreeGenerator.hpp:28-82).  Here a row block's LCS rectangle never leaves
// HBM as numbers: three small kernels turn it into the block's final bytes --
//   text_len_kernel   one workgroup per (row, segment of 1024 values): the segment's text length
//   text_scan_*       within-row prefix (one wave per row), then the rows' start offsets (one workgroup)
//   text_write_kernel the same workgroups again: every thread formats its 4 values into LDS at the scanned offsets,
//                     the workgroup copies the segment to its place with aligned 16-byte stores
// Bound: nothing on the chip (9 B of text per 2 B read; a block's kernels take well under a millisecond per 100 MB);
// the stage is bound by the host's write of the text.  All arithmetic that decides a byte is the reference's, in the
// reference's types and order: double division on the host-built pow table, round to float, back to double,
// a = (int64) v, b = (int64) ((1.0 + (v - a)) * 1e6 + 0.5) without contraction (-ffp-contract=off), the conversion of
// an out-of-range double as x86-64's cvttsd2si does it (INT64_MIN), so the lcs == 0 value prints as
// 9223372036854775808.223372036854775808 here too.
// The same passes serve lcsgpu_dist_text_batch, the rows of many small matrices in one launch sequence (text_group_*_kernel,
// tables from text_plan.h): a workgroup there is one (row, segment) job of the call, its values come straight out of its
// list's triangle or square, and the rows of all lists are scanned together.  What decides a byte is defined once, for both.
#include "lcs_kernels.h"

namespace lcsgpu {

namespace {

using lcsgpu_impl::TEXT_THREADS; // the shape of a text workgroup: text_plan.h
using lcsgpu_impl::TEXT_PER_THREAD;
using lcsgpu_impl::TEXT_SEG; // values per workgroup
constexpr int TEXT_MAX_VALUE = 39; // 19 + '.' + 18 digits + separator: the saturated value
constexpr int TEXT_LDS = TEXT_SEG * TEXT_MAX_VALUE + 32;

// (int64) v as the reference's x86-64 build converts (cvttsd2si): out of range or NaN -> INT64_MIN
__device__ __forceinline__ long long trunc_i64(double v)
{
    if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0)) return (long long)0x8000000000000000ull;
    return (long long)v;
}

__device__ __forceinline__ int n_digits(unsigned long long v)
{
    if (v <= 0xFFFFFFFFull) {
        uint32_t x = (uint32_t)v;
        int n = 1;
        while (x >= 10u) {
            x /= 10u;
            ++n;
        }
        return n;
    }
    int n = 1;
    while (v >= 10ull) {
        v /= 10ull;
        ++n;
    }
    return n;
}

// the decimal digits of v, the last one at p[end - 1]
__device__ __forceinline__ void put_digits(char* p, int end, unsigned long long v)
{
    while (v > 0xFFFFFFFFull) {
        p[--end] = (char)('0' + (int)(v % 10ull));
        v /= 10ull;
    }
    uint32_t x = (uint32_t)v;
    do {
        p[--end] = (char)('0' + (int)(x % 10u));
        x /= 10u;
    } while (x);
}

struct Parts {
    unsigned long long a, b;
    int na, nb;
};

// Double2PChar(v, 6): the two integers it prints and how many digits each has
__device__ __forceinline__ Parts split_value(float f)
{
    const double v = (double)f;
    const long long a = trunc_i64(v);
    const long long b = trunc_i64((1.0 + (v - (double)a)) * 1000000.0 + 0.5);
    Parts p;
    p.a = (unsigned long long)a;
    p.b = (unsigned long long)b;
    p.na = n_digits(p.a);
    p.nb = n_digits(p.b);
    return p;
}

// Transform<double, kind> -> float, or (kind 2) Transform<float, pairwise_identity>, of one LCS value
__device__ __forceinline__ float value_from(int kind, const double* __restrict__ pow_f64, uint32_t l, uint32_t len_i, uint32_t len_j)
{
    if (kind == 2) return (float)l / (float)(len_i < len_j ? len_i : len_j); // Transform<float, pairwise_identity>
    const uint32_t indel = len_i + len_j - 2u * l;
    double d;
    if (l == 0) d = 1.7976931348623155e308; // nextafter(DBL_MAX, 0), hpp:61,73
    else d = kind == 1 ? pow_f64[indel] / (double)l : (double)indel / (double)l;
    return (float)d; // the reference stores the row as floats before printing
}

// What a workgroup knows of its row, whichever launch it belongs to: cols values, value j = LCS lcs(j) against a sequence
// of len(j) residues.  BlockRow: a row of a block's rectangle (launch_text_block); GroupRow: a row of one list of a batched
// call, straight out of the list's packed triangle or square (launch_text_group_*).
template <typename T>
struct BlockRow {
    const T* lcs_row;
    const int32_t* where;
    const uint32_t* lens;
    int32_t cols;
    uint32_t len_i;
    __device__ __forceinline__ uint32_t lcs(int32_t j) const { return lcs_row[where ? where[j] : j]; }
    __device__ __forceinline__ uint32_t len(int32_t j) const { return lens[j]; }
};
struct GroupRow {
    const uint16_t* src;      // the row's first value
    const int32_t* members;   // the ids of the row's list
    const uint32_t* lens;
    int32_t cols;
    uint32_t len_i;
    __device__ __forceinline__ uint32_t lcs(int32_t j) const { return src[j]; }
    __device__ __forceinline__ uint32_t len(int32_t j) const { return lens[members[j]]; }
};

template <typename T>
__device__ __forceinline__ BlockRow<T> block_row(const TextArgs& t, int r)
{
    const int32_t i = t.row_begin + r;
    return BlockRow<T>{(const T*)t.lcs + (int64_t)r * t.ld, t.where, t.lens, t.square ? t.n : i, t.lens[i]};
}
__device__ __forceinline__ GroupRow group_row(const TextGroupArgs& g, const lcsgpu_impl::TextRow& R)
{
    return GroupRow{g.lcs + R.src, g.ids + R.pos0, g.lens, R.cols, g.lens[g.ids[R.pos]]};
}

template <class Row>
__device__ __forceinline__ float value_of(const Row& row, int kind, const double* __restrict__ pow_f64, int32_t j)
{
    return value_from(kind, pow_f64, row.lcs(j), row.len_i, row.len(j));
}

// The text length of segment `seg` of a row, without the row's name: valid in thread 0.
template <class Row>
__device__ __forceinline__ uint32_t segment_length(const Row& row, int kind, const double* __restrict__ pow_f64, int seg)
{
    const int32_t j0 = seg * TEXT_SEG + (int)threadIdx.x * TEXT_PER_THREAD;
    uint32_t mine = 0;
    for (int k = 0; k < TEXT_PER_THREAD; ++k) {
        const int32_t j = j0 + k;
        if (j >= row.cols) break;
        const Parts p = split_value(value_of(row, kind, pow_f64, j));
        mine += (uint32_t)(p.na + p.nb + 1); // the '.' takes the place of b's first digit; + the separator
    }
    for (int off = 32; off; off >>= 1) mine += __shfl_down(mine, off, 64);
    __shared__ uint32_t part[TEXT_THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    uint32_t sum = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < TEXT_THREADS / 64; ++w) sum += part[w];
    return sum;
}

// one wave: s[0 .. count) -> exclusive prefix (in place); returns the sum
__device__ __forceinline__ uint32_t scan_row_segments(uint32_t* s, int count, int lane)
{
    uint32_t run = 0;
    for (int base = 0; base < count; base += 64) {
        const int k = base + lane;
        const uint32_t v = k < count ? s[k] : 0u;
        uint32_t inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (k < count) s[k] = run + inc - v;
        run += __shfl(inc, 63, 64);
    }
    return run;
}

// Segment `seg` of a row to out + dst (where the segment starts; for segment 0: where the row does): the row's name with
// its separator straight to memory, then every thread formats its values into LDS at the scanned offsets and the workgroup
// copies the segment to its place with aligned 16-byte stores.
template <class Row>
__device__ __forceinline__ void write_segment(const Row& row, int kind, const double* __restrict__ pow_f64, int seg, char* __restrict__ out,
                                              unsigned long long dst, const char* __restrict__ name, unsigned long long id_len)
{
    __shared__ __align__(16) char lds[TEXT_LDS];
    __shared__ uint32_t wave_sum[TEXT_THREADS / 64];
    const int32_t cols = row.cols;
    if (seg == 0) { // the row's id and its separator, straight to memory
        for (unsigned long long k = threadIdx.x; k < id_len; k += TEXT_THREADS) out[dst + k] = name[k];
        if (threadIdx.x == 0) out[dst + id_len] = cols == 0 ? '\n' : ',';
        dst += id_len + 1;
    }
    const int32_t j0 = seg * TEXT_SEG + (int)threadIdx.x * TEXT_PER_THREAD;
    Parts p[TEXT_PER_THREAD];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < TEXT_PER_THREAD; ++k) {
        const int32_t j = j0 + k;
        if (j < cols) {
            p[k] = split_value(value_of(row, kind, pow_f64, j));
            mine += (uint32_t)(p[k].na + p[k].nb + 1);
        } else {
            p[k].na = p[k].nb = 0;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < TEXT_THREADS / 64; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    // LDS byte k + mis <-> output byte dst + k: the copy below then moves whole aligned 16-byte words
    const uint32_t mis = (uint32_t)((unsigned long long)(uintptr_t)(out + dst) & 15ull);
    uint32_t at = mis + before + inc - mine;
#pragma unroll
    for (int k = 0; k < TEXT_PER_THREAD; ++k) {
        if (p[k].na == 0) continue;
        put_digits(lds, (int)at + p[k].na, p[k].a);
        put_digits(lds, (int)at + p[k].na + p[k].nb, p[k].b);
        lds[at + p[k].na] = '.'; // over b's leading digit
        at += (uint32_t)(p[k].na + p[k].nb);
        lds[at++] = (j0 + k == cols - 1) ? '\n' : ',';
    }
    __syncthreads();
    char* const base = out + dst - mis; // 16-byte aligned
    const uint32_t end = mis + total, words = (end + 15u) / 16u;
    for (uint32_t w = threadIdx.x; w < words; w += TEXT_THREADS) {
        const uint32_t b0 = w * 16u;
        if (b0 >= mis && b0 + 16u <= end) {
            *reinterpret_cast<uint4*>(base + b0) = *reinterpret_cast<const uint4*>(lds + b0);
        } else {
            const uint32_t lo = b0 < mis ? mis : b0, hi = b0 + 16u < end ? b0 + 16u : end;
            for (uint32_t b = lo; b < hi; ++b) base[b] = lds[b];
        }
    }
}

// ---- a row block of one set (launch_text_block) ----

template <typename T>
__global__ __launch_bounds__(TEXT_THREADS) void text_len_kernel(TextArgs t)
{
    const int seg = blockIdx.x, r = blockIdx.y;
    const int32_t i = t.row_begin + r;
    uint32_t sum = segment_length(block_row<T>(t, r), t.kind, t.pow_f64, seg);
    if (threadIdx.x == 0) {
        if (seg == 0) sum += (uint32_t)(t.id_off[i + 1] - t.id_off[i]) + 1u; // "<id>," (or "<id>\n" for an empty row)
        t.seg_len[(int64_t)r * t.segs + seg] = sum;
    }
}

// one wave per row: seg_len -> exclusive prefix inside the row (in place), row_len = the row's bytes
__global__ __launch_bounds__(256) void text_scan_rows_kernel(TextArgs t)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= t.n_rows) return;
    const uint32_t run = scan_row_segments(t.seg_len + (int64_t)r * t.segs, t.segs, lane);
    if (lane == 0) t.row_len[r] = run;
}

// one workgroup: row_len -> row_start (exclusive, 64-bit), row_start[n_rows] = the bytes of all rows
__global__ __launch_bounds__(1024) void text_scan_block_kernel(const uint32_t* __restrict__ row_len, unsigned long long* __restrict__ row_start,
                                                               int n_rows)
{
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_rows; base += 1024) {
        const int r = base + threadIdx.x;
        const unsigned long long v = r < n_rows ? (unsigned long long)row_len[r] : 0ull;
        unsigned long long inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (r < n_rows) row_start[r] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) row_start[n_rows] = carry;
}

template <typename T>
__global__ __launch_bounds__(TEXT_THREADS) void text_write_kernel(TextArgs t)
{
    const int seg = blockIdx.x, r = blockIdx.y;
    const int32_t i = t.row_begin + r;
    const BlockRow<T> row = block_row<T>(t, r);
    if (seg > 0 && (int64_t)seg * TEXT_SEG >= row.cols) return;
    const unsigned long long dst = t.row_start[r] + t.seg_len[(int64_t)r * t.segs + seg];
    const unsigned long long b0 = t.id_off[i];
    write_segment(row, t.kind, t.pow_f64, seg, t.out, dst, t.ids + b0, t.id_off[i + 1] - b0);
}

// ---- the rows of many lists in one launch sequence (launch_text_group_*): workgroup b = job b of the call's plan
// (text_plan.h): one load tells it its row, the row's record the rest.  Nothing waits for another workgroup, there are no
// atomics, and every loop bound is a column count or a table length fixed at launch. ----

__global__ __launch_bounds__(TEXT_THREADS) void text_group_len_kernel(TextGroupArgs g)
{
    const int b = blockIdx.x;
    const lcsgpu_impl::TextRow R = g.rows[g.job_row[b]];
    const int seg = b - R.job0;
    uint32_t sum = segment_length(group_row(g, R), g.kind, g.pow_f64, seg);
    if (threadIdx.x == 0) {
        const int32_t id = g.ids[R.pos];
        if (seg == 0) sum += (uint32_t)(g.name_off[id + 1] - g.name_off[id]) + 1u; // "<name>," (or "<name>\n" for an empty row)
        g.seg_len[b] = sum;
    }
}

// one wave per row, as text_scan_rows_kernel: the row's segments are the jobs [job0, the next row's job0)
__global__ __launch_bounds__(256) void text_group_scan_rows_kernel(TextGroupArgs g)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= g.n_rows) return;
    const int32_t j0 = g.rows[r].job0, j1 = g.rows[r + 1].job0;
    const uint32_t run = scan_row_segments(g.seg_len + j0, j1 - j0, lane);
    if (lane == 0) g.row_len[r] = run;
}

// where every list's text starts; [n_groups] = the bytes of the call
__global__ __launch_bounds__(256) void text_group_list_start_kernel(TextGroupArgs g)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l <= g.n_groups) g.list_start[l] = g.row_start[g.list_row0[l]];
}

__global__ __launch_bounds__(TEXT_THREADS) void text_group_write_kernel(TextGroupArgs g)
{
    const int b = blockIdx.x;
    const int32_t r = g.job_row[b];
    const lcsgpu_impl::TextRow R = g.rows[r];
    const int seg = b - R.job0;
    const int32_t id = g.ids[R.pos];
    const unsigned long long n0 = g.name_off[id];
    write_segment(group_row(g, R), g.kind, g.pow_f64, seg, g.out, g.row_start[r] + g.seg_len[b], g.names + n0, g.name_off[id + 1] - n0);
}

} // namespace

hipError_t launch_text_block(const TextArgs& t, hipStream_t stream)
{
    if (t.n_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)t.segs, (unsigned)t.n_rows);
    if (t.elem_size == 2) hipLaunchKernelGGL(text_len_kernel<uint16_t>, grid, dim3(TEXT_THREADS), 0, stream, t);
    else hipLaunchKernelGGL(text_len_kernel<uint32_t>, grid, dim3(TEXT_THREADS), 0, stream, t);
    hipLaunchKernelGGL(text_scan_rows_kernel, dim3((unsigned)((t.n_rows + 3) / 4)), dim3(256), 0, stream, t);
    hipLaunchKernelGGL(text_scan_block_kernel, dim3(1), dim3(1024), 0, stream, (const uint32_t*)t.row_len, t.row_start, t.n_rows);
    if (t.elem_size == 2) hipLaunchKernelGGL(text_write_kernel<uint16_t>, grid, dim3(TEXT_THREADS), 0, stream, t);
    else hipLaunchKernelGGL(text_write_kernel<uint32_t>, grid, dim3(TEXT_THREADS), 0, stream, t);
    return hipGetLastError();
}

// The batched form up to the sizes: every segment's length, the prefix inside every row, the prefix over all rows of the
// call -- text_scan_block_kernel, ONE workgroup that takes 1024 rows per trip: a trip is three barriers and a 64-lane scan,
// a microsecond or two, so 500 000 rows (a chunk of 10 000 families of 50) are about a millisecond in a call whose LCS and
// write launches take tens; no two-level form -- and every list's start with the total behind.
hipError_t launch_text_group_lengths(const TextGroupArgs& g, hipStream_t stream)
{
    if (g.n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(text_group_len_kernel, dim3((unsigned)g.n_jobs), dim3(TEXT_THREADS), 0, stream, g);
    hipLaunchKernelGGL(text_group_scan_rows_kernel, dim3((unsigned)((g.n_rows + 3) / 4)), dim3(256), 0, stream, g);
    hipLaunchKernelGGL(text_scan_block_kernel, dim3(1), dim3(1024), 0, stream, (const uint32_t*)g.row_len, g.row_start, g.n_rows);
    hipLaunchKernelGGL(text_group_list_start_kernel, dim3((unsigned)(g.n_groups / 256 + 1)), dim3(256), 0, stream, g);
    return hipGetLastError();
}

// ... and the write pass into g.out, which holds list_start[n_groups] bytes
hipError_t launch_text_group_write(const TextGroupArgs& g, hipStream_t stream)
{
    if (g.n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(text_group_write_kernel, dim3((unsigned)g.n_jobs), dim3(TEXT_THREADS), 0, stream, g);
    return hipGetLastError();
}

int text_segment_values() { return TEXT_SEG; }
int text_max_value_bytes() { return TEXT_MAX_VALUE; }

} // namespace lcsgpu
