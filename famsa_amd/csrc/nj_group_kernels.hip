// nj_group_kernels.hip -- NeighborJoining::computeTree (reference tree/NeighborJoining.cpp:33-118) of MANY small groups, ONE
// WORKGROUP PER GROUP (lcsgpu_nj_batch): the batched form of nj_loop_kernels.hip, built the way upgma_group_kernels.hip is.
// The resident launch of lcsgpu_nj spreads ONE tree over the chip and pays an exchange between workgroups per merge; a
// family of a few hundred members is better off alone on a CU, beside 255 others.
//
// A slice of groups is a launch pair (a triple when it holds groups on both sides of the thread-count switch):
//   nj_group_dist_kernel   one workgroup per matrix row i: the group's packed uint16 LCS triangle into its packed FLOAT
//                          triangle (Transform<float, kind>, the expressions of launch_float_distances; the scan looks at
//                          i < j only, so the triangle is enough), and, while the whole row is in LDS, the row's initial
//                          sum: every other distance added in ascending index, as one wave's ordered sum (ordered_sum.h:
//                          bit for bit the one-after-the-other float additions).
//   nj_group_kernel        one workgroup per group, longest first: the m - 2 merges and the last record.
//
// STATE.  The live clusters are kept COMPACT and in ascending row order, as the reference's vector with its erase() keeps
// them: per POSITION p the row (uint16), the node id (uint16, below 2 * 2048) and the sum (float), 8 B per row, in two
// copies that alternate by merge parity (a merge reads one and writes the other, so removing a position is a shifted
// copy and needs no barrier of its own), plus the merged row's new distances (the addends of its sum): 41 KB at the cap.
// A dead row is never looked at again; the float triangle keeps its layout by ORIGINAL row (never squeezed): a live row's
// live columns are a gather with holes, still mostly whole cache lines.  Positions ascend with rows, so "first strict
// minimum over i < j in lexicographic order of the live clusters" is the smallest (q, position i, position j).
//
// A MERGE, three barriers:
//   1  SCAN.  Columns in chunks of 64 positions (lane = column: its row and sum stay in registers for the chunk), the
//      rows below the chunk dealt to the waves round robin.  A wave fetches the rows and sums of 64 of its positions with
//      one LDS read per lane and takes them out of the registers as scalars (v_readlane): with an LDS round trip per
//      row the scan waited for exactly that (256 threads: 87.6 against 53.9 ms at 1000 members; 1024: 36.5 against 33.8).  Eight rows' loads are in
//      flight together, all unconditional (a lane without a pair reads an element that exists and ignores it).  A thread meets its pairs in
//      ascending (i, j), so a strict '<' against a best that starts at FLT_MAX keeps its first strict minimum; a NaN never
//      wins.  Then the wave's (q, i << 16 | j) by DPP, one slot per wave, ONE barrier, and every thread reads all slots.
//      No q below FLT_MAX: the group's status becomes 1 and the workgroup leaves -- every thread decides that from the
//      same slots.
//   2  UPDATE.  Thread t takes the positions k = t, t + THREADS, ...: both loads D(i, k), D(j, k) first, then
//      sum_k -= (Dik + Djk); Dik = (Dik + Djk - Dij) / 2; sum_k += Dik -- written to the other copy at k's new position.
//   3  CHAIN.  Wave 0 adds the new Dik up in ascending k from 0 (wave_ordered_sum over the addends in LDS; positions i
//      and beyond the end hold +0.0f, which changes no float sum that started at +0.0f) -> the merged row's sum.
// What crosses threads in memory is the triangle: D(i, k) is stored by k's owner and read by anybody in the next scan,
// two barriers later (a workgroup-scope fence each; the workgroup sits on one CU and its plain loads and stores go through
// the same vector L1, as in upgma_group_kernel).
// No workgroup waits for another, every loop bound is known at launch or shrinks with the merge counter, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpp_min.h"
#include "fasttree_kernels.h"
#include "ordered_sum.h"

namespace lcsgpu {

namespace {

constexpr uint32_t NJG_NONE = 0xFFFFFFFFu;
constexpr float NJG_QMAX = 3.40282347e38f; // numeric_limits<float>::max(): only a q below it can win
constexpr int NJG_PAD = ordered_sum_padded(NJ_GROUP_MAX_MEMBERS);
constexpr int NJG_UNROLL = 8; // rows of a wave whose loads are in flight together
static_assert(64 % NJG_UNROLL == 0, "a block of 64 rows is whole batches");

__device__ __forceinline__ bool njg_less(float q2, uint32_t k2, float q, uint32_t k) { return q2 < q || (q2 == q && k2 < k); }

// TriangleMatrix::access for lo < hi (both below 2048: the index stays below 2^21)
__device__ __forceinline__ int njg_tri(int lo, int hi) { return hi * (hi - 1) / 2 + lo; }

__host__ __device__ constexpr int njg_cap(int max_m) { return (max_m + 7) & ~7; }

} // namespace

__global__ __launch_bounds__(256) void nj_group_dist_kernel(GroupNjArgs a)
{
    __shared__ float s_row[NJG_PAD];
    // which job this row belongs to: the last one whose first row is <= the block's
    const int64_t row = blockIdx.x;
    int lo = 0, hi = a.n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.row0[mid] <= row) lo = mid; else hi = mid - 1;
    }
    const GroupNjJob job = a.jobs[lo];
    const int m = job.m, i = (int)(row - a.row0[lo]);
    if (i >= m || m > NJ_GROUP_MAX_MEMBERS) return; // (uniform; cannot happen: the grid is row0[n_jobs])
    const uint16_t* tri = a.tri + job.tri0;
    const int32_t* ids = a.ids + job.id0;
    float* out = a.dist + job.f0 + (int64_t)i * (i - 1) / 2;
    const uint32_t len_i = a.lens[ids[i]];
    const int padded = ordered_sum_padded(m);
    for (int j = threadIdx.x; j < padded; j += 256) {
        float d = 0.0f; // the diagonal and the padding: +0.0f changes no sum
        if (j < m && j != i) {
            const int h = i > j ? i : j, l = i > j ? j : i;
            const uint32_t lcs = tri[njg_tri(l, h)];
            const uint32_t indel = len_i + a.lens[ids[j]] - 2u * lcs;
            if (lcs == 0)
                d = 3.40282347e38f; // (float) nextafter((double) FLT_MAX, 0) rounds back to FLT_MAX
            else if (a.kind == 1)
                d = __fdiv_rn(a.pow_f32[indel], (float)lcs);
            else
                d = __fdiv_rn((float)indel, (float)lcs);
            if (j < i) out[j] = d;
        }
        s_row[j] = d;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const float s = wave_ordered_sum(s_row, m);
        if (threadIdx.x == 0) a.row_sum[row] = s;
    }
}

constexpr size_t group_nj_lds_bytes(int threads, int max_m)
{
    // the waves' slots, the addends of the chain, then two copies of the positions: sum, row, node
    return (size_t)(threads / 64) * 8 + (size_t)ordered_sum_padded(max_m) * 4 + (size_t)2 * njg_cap(max_m) * 8;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void nj_group_kernel(GroupNjArgs a, int first_job)
{
    constexpr int WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_nj[];
    const int cap = njg_cap(a.max_m);
    uint2* const s_slot = (uint2*)s_nj;                                  // [WAVES]
    float* const s_tmp = (float*)(s_slot + WAVES);                       // [ordered_sum_padded(max_m)]
    float* const s_sum = s_tmp + ordered_sum_padded(a.max_m);            // [2][cap]
    uint16_t* const s_rowid = (uint16_t*)(s_sum + 2 * cap);              // [2][cap]
    uint16_t* const s_node = s_rowid + 2 * cap;                          // [2][cap]

    const int jb = first_job + (int)blockIdx.x;
    const GroupNjJob job = a.jobs[jb];
    const int m = job.m;
    if (m > a.max_m || m > NJ_GROUP_MAX_MEMBERS || m < 2) return; // (uniform; cannot happen)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const D = a.dist + job.f0;
    const int64_t r0 = a.row0[jb];

    for (int k = tid; k < m; k += THREADS) {
        s_sum[k] = a.row_sum[r0 + k];
        s_rowid[k] = (uint16_t)k;
        s_node[k] = (uint16_t)k;
    }
    for (int k = tid; k < ordered_sum_padded(m); k += THREADS) s_tmp[k] = 0.0f;
    __syncthreads();

    int step = 0;
    for (int L = m; L > 2; --L, ++step) {
        const int cur = (step & 1) * cap, nxt = cap - cur;
        const float* const sum_c = s_sum + cur;
        const uint16_t* const row_c = s_rowid + cur;
        const uint16_t* const node_c = s_node + cur;

        // ---- 1: the smallest q over the live pairs ----
        const float f = (float)(L - 2);
        float bq = NJG_QMAX;
        uint32_t bkey = NJG_NONE;
        for (int c0 = 0; c0 < L - 1; c0 += 64) {
            const int px = c0 + lane;
            const bool col = px < L - 1;
            const int rx = col ? row_c[px] : 0;
            const float sx = col ? sum_c[px] : 0.0f;
            // a block of up to 64 of the wave's rows: lane l fetches the row and the sum of position pyb + l * WAVES once, the
            // loop below takes them out of the registers as scalars (no trip to LDS per row)
            for (int pyb = c0 + 1 + wave; pyb < L; pyb += 64 * WAVES) {
                const int pyl = pyb + lane * WAVES, pylc = pyl < L ? pyl : L - 1;
                const int rowv = row_c[pylc];
                const int sumv = __float_as_int(sum_c[pylc]);
                const int n_rows = min(64, (L - pyb + WAVES - 1) / WAVES);
                for (int u0 = 0; u0 < n_rows; u0 += NJG_UNROLL) { // (u0 + NJG_UNROLL <= 64)
                    float d[NJG_UNROLL], sy[NJG_UNROLL];
                    bool ok[NJG_UNROLL];
#pragma unroll
                    for (int u = 0; u < NJG_UNROLL; ++u) { // the loads first, all of them unconditional
                        const int py = pyb + (u0 + u) * WAVES;
                        ok[u] = py < L && px < py;
                        // a lane beyond the rows holds the last live row: always a row >= 1, whose element min(rx, ry - 1)
                        // exists -- what a lane without a pair loads (and then ignores)
                        const int ry = __builtin_amdgcn_readlane(rowv, u0 + u);
                        sy[u] = __int_as_float(__builtin_amdgcn_readlane(sumv, u0 + u));
                        d[u] = D[njg_tri(0, ry) + min(rx, ry - 1)];
                    }
#pragma unroll
                    for (int u = 0; u < NJG_UNROLL; ++u) {
                        const float q = __fsub_rn(__fsub_rn(__fmul_rn(f, d[u]), sx), sy[u]);
                        if (ok[u] && q < bq) { bq = q; bkey = (uint32_t)px << 16 | (uint32_t)(pyb + (u0 + u) * WAVES); }
                    }
                }
            }
        }
        wave_first_min(bq, bkey);
        if (lane == 0) s_slot[wave] = make_uint2(__float_as_uint(bq), bkey);
        __syncthreads();
        float gq = NJG_QMAX;
        uint32_t gkey = NJG_NONE;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint2 s = s_slot[w];
            if (njg_less(__uint_as_float(s.x), s.y, gq, gkey)) { gq = __uint_as_float(s.x); gkey = s.y; }
        }
        const int pi = (int)(gkey >> 16), pj = (int)(gkey & 0xFFFFu);
        if (!(gq < NJG_QMAX) || pi >= pj || pj >= L) { // uniform: every thread read the same slots
            if (tid == 0) a.status[job.group] = 1;
            return;
        }

        // ---- 2: the merged row's distances, everybody's sums; position pj leaves ----
        const int ra = row_c[pi], rb = row_c[pj];
        const float dab = D[njg_tri(ra, rb)];
        for (int k = tid; k < L; k += THREADS) {
            if (k == pj) continue;
            const int kk = k - (k > pj ? 1 : 0);
            if (k == pi) {
                a.left[job.node0 + step] = node_c[pi];
                a.right[job.node0 + step] = node_c[pj];
                s_rowid[nxt + kk] = (uint16_t)ra;
                s_node[nxt + kk] = (uint16_t)(m + step);
                s_tmp[kk] = 0.0f;
                continue;
            }
            const int rk = row_c[k];
            float* const pa = D + (rk < ra ? njg_tri(rk, ra) : njg_tri(ra, rk));
            const float* const pb = D + (rk < rb ? njg_tri(rk, rb) : njg_tri(rb, rk));
            const float x = *pa, y = *pb;
            const float u = __fadd_rn(x, y);
            const float nd = __fmul_rn(__fsub_rn(u, dab), 0.5f); // (Dik + Djk - Dij) / 2: halving is exact or rounds as the division does
            s_sum[nxt + kk] = __fadd_rn(__fsub_rn(sum_c[k], u), nd);
            s_rowid[nxt + kk] = (uint16_t)rk;
            s_node[nxt + kk] = node_c[k];
            s_tmp[kk] = nd;
            *pa = nd;
        }
        if (tid == 0) s_tmp[L - 1] = 0.0f; // the last position of the merge before: beyond the end now
        __syncthreads();

        // ---- 3: the merged row's sum, in ascending order ----
        if (wave == 0) {
            const float s = wave_ordered_sum(s_tmp, L - 1);
            if (lane == 0) s_sum[nxt + pi] = s;
        }
        __syncthreads();
    }
    if (tid == 0) { // the two clusters left
        const int cur = (step & 1) * cap;
        a.left[job.node0 + step] = s_node[cur];
        a.right[job.node0 + step] = s_node[cur + 1];
    }
}

int group_nj_launches(const GroupNjArgs& a)
{
    if (a.n_jobs <= 0) return 0;
    return 1 + (a.n_wide > 0 ? 1 : 0) + (a.n_wide < a.n_jobs ? 1 : 0);
}

hipError_t launch_group_nj(const GroupNjArgs& a, hipStream_t stream)
{
    if (a.n_jobs <= 0) return hipSuccess;
    if (a.max_m < 2 || a.max_m > NJ_GROUP_MAX_MEMBERS) return hipErrorInvalidValue;
    if (a.total_rows <= 0 || a.total_rows > 0x7fffffff) return hipErrorInvalidValue;
    if (a.n_wide < 0 || a.n_wide > a.n_jobs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nj_group_dist_kernel, dim3((unsigned)a.total_rows), dim3(256), 0, stream, a);
    if (a.n_wide > 0)
        hipLaunchKernelGGL((nj_group_kernel<1024>), dim3((unsigned)a.n_wide), dim3(1024), group_nj_lds_bytes(1024, a.max_m), stream, a, 0);
    if (a.n_wide < a.n_jobs) {
        GroupNjArgs b = a; // the LDS of the narrow groups follows their own longest
        b.max_m = a.n_wide > 0 ? a.narrow_m : a.max_m;
        if (b.max_m < 2 || b.max_m > a.max_m) return hipErrorInvalidValue;
        hipLaunchKernelGGL((nj_group_kernel<256>), dim3((unsigned)(a.n_jobs - a.n_wide)), dim3(256), group_nj_lds_bytes(256, b.max_m), stream, b,
                           a.n_wide);
    }
    return hipGetLastError();
}

} // namespace lcsgpu
