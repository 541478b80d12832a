// upgma_group_kernels.hip -- UPGMA::computeTree (reference tree/UPGMA.cpp:114-295) of MANY small groups, ONE WORKGROUP PER
// GROUP (lcsgpu_upgma_batch): the guide trees of a batch of families side by side, as mst_group_prim_kernel
// (mst_kernels.hip) does it for -gt sl.  The big-tree forms (tree_kernels.hip: a launch per merge; upgma_batch_kernels.hip:
// several merges per three launches) pay launches per merge, which is all a tree of a few hundred members costs them.
//
// A slice of groups is a launch pair:
//   upgma_group_dist_kernel   one workgroup per matrix row: the group's packed uint16 LCS triangle into its m x m
//                             symmetric float square (Transform<float, kind>, the expression of upgma_dist_square_kernel),
//                             and, while the row is in registers, the row's initial key.
//   upgma_group_kernel        one workgroup per group, longest first: the m - 1 merges.
//
// INITIAL KEYS.  The reference's double loop (UPGMA.cpp:198-215) offers d(i, j), j < i, to row i and to row j, i ascending
// outside, j ascending inside, both with a strict '<'.  Row r therefore sees its candidates in this order: at i = r the
// columns 0 .. r - 1 ascending, then at i = r + 1, r + 2, ... the column i -- every other row once, in ascending index --
// and keeps the first strict minimum below BIG_DIST.  That is "the smallest (d, index) over the whole row", which the
// dist kernel reduces while it writes the row.
//
// A STEP.  Per-row state in LDS: min_dist (float), nearest (uint16), node index (uint16, DEAD = the row left) -- 8 B per
// row, 32 KB at the cap.  Row j's state belongs to thread j % THREADS (at most four rows per thread); what crosses threads:
//   * the waves' partial minima, in two sets of slots alternating by step parity (a set is written again only two
//     barriers after anybody read it), so ONE barrier per step is enough;
//   * nearest[Lmin] of the row picked next, written by its owner before the barrier, read by everybody after it;
//   * the matrix: the merged row `keep` is written by the threads that own the COLUMNS (D[keep][j], and its mirror
//     D[j][keep]); when row j is merged later, D[j][keep] is read by the owner of column keep -- a different thread.  The
//     step's __syncthreads() (a workgroup-scope fence: the workgroup sits on one CU, its stores and loads go through the
//     same vector L1) is what makes those plain stores visible; a thread never reads another thread's store of the SAME
//     step, because a step reads rows Lmin / Rmin at the columns it owns and writes only those columns and their mirrors.
// Before the barrier a thread reduces two keys in one pass over its rows j (alive, not Lmin / Rmin): the smallest new
// value (the merged row's key: first strict minimum below BIG_DIST in ascending j) and the smallest STALE key
// (min_dist[j], j).  After the one exchange every thread derives the next pick as the smaller of "best stale key" and
// "(new key, Lmin)" -- the other rows' min_dist are deliberately not refreshed, as in the reference: that staleness
// decides topologies.  All distances are >= 0 or FLT_MAX / +inf, never NaN (no subtraction anywhere), so "first strict
// minimum in ascending index" is the smallest (value, index) pair.
// When no alive row has a key below BIG_DIST the reference's behaviour is undefined; the workgroup sets the group's
// status and returns -- every thread takes that decision from the same slots, after the barrier.
// No workgroup waits for another, every loop bound is known at launch, there are no atomics.
// Heights and branch lengths are not computed: the Newick texts of this project carry none.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpp_min.h"
#include "fasttree_kernels.h"

namespace lcsgpu {

namespace {

constexpr uint32_t G_NONE = 0x7FFFFFFFu;
constexpr float G_BIG = 1e29f; // UPGMA::BIG_DIST, reference tree/UPGMA.h:106
constexpr uint16_t G_DEAD = 0xFFFFu;
constexpr int G_ROWS = 4; // rows of a thread: UPGMA_GROUP_MAX_MEMBERS / 1024 threads, 1024 members / 256 threads

__device__ __forceinline__ bool first_min_less(float d2, uint32_t j2, float d, uint32_t j)
{
    return d2 < d || (d2 == d && j2 < j);
}

} // namespace

__global__ __launch_bounds__(256) void upgma_group_dist_kernel(GroupUpgmaArgs a)
{
    __shared__ float s_d[4];
    __shared__ uint32_t s_j[4];
    // which job this row belongs to: the last one whose first row is <= the block's
    const int64_t row = blockIdx.x;
    int lo = 0, hi = a.n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.row0[mid] <= row) lo = mid; else hi = mid - 1;
    }
    const GroupUpgmaJob job = a.jobs[lo];
    const int m = job.m, i = (int)(row - a.row0[lo]);
    if (i >= m) return; // (uniform; cannot happen: the grid is row0[n_jobs])
    const uint16_t* tri = a.tri + job.tri0;
    const int32_t* ids = a.ids + job.id0;
    float* out = a.sq + job.sq0 + (int64_t)i * m;
    const uint32_t len_i = a.lens[ids[i]];
    float best = G_BIG;
    uint32_t bj = G_NONE;
    for (int j = threadIdx.x; j < m; j += 256) {
        float d = 0.0f; // the diagonal is never read; keep it defined
        if (j != i) {
            const int64_t h = i > j ? i : j, l = i > j ? j : i;
            const uint32_t lcs = tri[h * (h - 1) / 2 + l];
            const uint32_t indel = len_i + a.lens[ids[j]] - 2u * lcs;
            if (lcs == 0)
                d = 3.40282347e38f; // (float) nextafter((double) FLT_MAX, 0) rounds back to FLT_MAX
            else if (a.kind == 1)
                d = __fdiv_rn(a.pow_f32[indel], (float)lcs);
            else
                d = __fdiv_rn((float)indel, (float)lcs);
            if (d < best) { best = d; bj = (uint32_t)j; } // ascending j, strict
        }
        out[j] = d;
    }
    wave_first_min(best, bj);
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = best; s_j[threadIdx.x >> 6] = bj; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (first_min_less(s_d[w], s_j[w], best, bj)) { best = s_d[w]; bj = s_j[w]; }
        a.row_min[row] = best;
        a.row_near[row] = (int32_t)bj;
    }
}

constexpr size_t group_upgma_lds_bytes(int threads, int cap)
{
    // the waves' two sets of (stale d, stale row, new d, new column), then the rows: min_dist, nearest, node
    return (size_t)2 * (threads / 64) * 16 + (size_t)cap * 8;
}

template <bool MODIFIED, int THREADS>
__global__ __launch_bounds__(THREADS) void upgma_group_kernel(GroupUpgmaArgs a)
{
    constexpr int WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_upgma[];
    uint4* s_slot = (uint4*)s_upgma;                  // [2][WAVES]
    float* s_min = (float*)(s_slot + 2 * WAVES);      // [max_m]
    uint16_t* s_near = (uint16_t*)(s_min + a.max_m);  // [max_m] (G_NONE is stored as 0xFFFF: never a row)
    uint16_t* s_node = s_near + a.max_m;              // [max_m]

    const GroupUpgmaJob job = a.jobs[blockIdx.x];
    const int m = job.m;
    if (m > G_ROWS * THREADS) return; // (uniform; the launcher chooses THREADS by the longest group)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const D = a.sq + job.sq0;
    const int64_t r0 = a.row0[blockIdx.x];

    // the rows' initial keys, and the first pick
    float sd = G_BIG, nd = G_BIG;
    uint32_t sj = G_NONE, nj = G_NONE;
#pragma unroll
    for (int k = 0; k < G_ROWS; ++k) {
        const int j = tid + k * THREADS;
        if (j < m) {
            const float mn = a.row_min[r0 + j];
            s_min[j] = mn;
            s_near[j] = (uint16_t)a.row_near[r0 + j];
            s_node[j] = (uint16_t)j;
            if (mn < sd) { sd = mn; sj = (uint32_t)j; }
        }
    }
    wave_first_min(sd, sj);
    if (lane == 0) s_slot[WAVES + wave] = make_uint4(__float_as_uint(sd), sj, __float_as_uint(G_BIG), G_NONE);
    __syncthreads();
    int L, R;
    {
        float gd = G_BIG;
        uint32_t gj = G_NONE;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint4 s = s_slot[WAVES + w];
            if (first_min_less(__uint_as_float(s.x), s.y, gd, gj)) { gd = __uint_as_float(s.x); gj = s.y; }
        }
        if (!(gd < G_BIG)) { // uniform: every thread read the same slots
            if (tid == 0) a.status[job.group] = 1;
            return;
        }
        L = (int)gj;
        R = s_near[L];
    }

    for (int step = 0; step + 1 < m; ++step) {
        if ((unsigned)L >= (unsigned)m || (unsigned)R >= (unsigned)m || L == R) { // (cannot happen: a key below BIG_DIST
            if (tid == 0) a.status[job.group] = 1;                                //  names an alive row; uniform)
            return;
        }
        const float* const rowL = D + (int64_t)L * m;
        const float* const rowR = D + (int64_t)R * m;
        float x[G_ROWS], y[G_ROWS];
        bool act[G_ROWS];
#pragma unroll
        for (int k = 0; k < G_ROWS; ++k) { // the loads first: a step is their latency
            const int j = tid + k * THREADS;
            act[k] = j < m && j != L && j != R && s_node[j] != G_DEAD;
            x[k] = act[k] ? rowL[j] : 0.0f;
            y[k] = act[k] ? rowR[j] : 0.0f;
        }
        sd = nd = G_BIG;
        sj = nj = G_NONE;
#pragma unroll
        for (int k = 0; k < G_ROWS; ++k) {
            const int j = tid + k * THREADS;
            if (!act[k]) continue;
            float v;
            if (MODIFIED) // 0.05f * (x + y) + 0.9f * min(x, y), no contraction (reference UPGMA.cpp:32-34)
                v = __fadd_rn(__fmul_rn(0.05f, __fadd_rn(x[k], y[k])), __fmul_rn(0.9f, fminf(x[k], y[k])));
            else
                v = __fmul_rn(__fadd_rn(x[k], y[k]), 0.5f);
            if (s_near[j] == (uint16_t)R) s_near[j] = (uint16_t)L;
            D[(int64_t)L * m + j] = v;
            D[(int64_t)j * m + L] = v; // the mirror: read after a later barrier by the owner of column L
            if (v < nd) { nd = v; nj = (uint32_t)j; }
            const float mn = s_min[j]; // stale on purpose
            if (mn < sd) { sd = mn; sj = (uint32_t)j; }
        }
        if (tid == (L & (THREADS - 1))) { // the owner of the kept row: the record, and both rows' node entries
            a.left[job.node0 + step] = s_node[L];
            a.right[job.node0 + step] = s_node[R];
            s_node[L] = (uint16_t)(m + step);
            s_node[R] = G_DEAD;
        }
        wave_first_min(sd, sj);
        wave_first_min(nd, nj);
        const int set = (step & 1) * WAVES;
        if (lane == 0) s_slot[set + wave] = make_uint4(__float_as_uint(sd), sj, __float_as_uint(nd), nj);
        __syncthreads();
        float gsd = G_BIG, gnd = G_BIG;
        uint32_t gsj = G_NONE, gnj = G_NONE;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint4 s = s_slot[set + w];
            if (first_min_less(__uint_as_float(s.x), s.y, gsd, gsj)) { gsd = __uint_as_float(s.x); gsj = s.y; }
            if (first_min_less(__uint_as_float(s.z), s.w, gnd, gnj)) { gnd = __uint_as_float(s.z); gnj = s.w; }
        }
        if (tid == (L & (THREADS - 1))) { // the merged row's key: (BIG_DIST, NONE) when it has no finite neighbour
            s_min[L] = gnd;
            s_near[L] = (uint16_t)gnj;
        }
        if (step + 2 >= m) break; // the root: nothing left to pick
        // the next pick: the smaller of the best stale key and the merged row's (nobody reads s_near[L] here: when the
        // merged row wins, its neighbour comes from the slots)
        if (gnd < G_BIG && first_min_less(gnd, (uint32_t)L, gsd, gsj)) {
            R = (int)gnj;
        } else if (gsd < G_BIG) {
            L = (int)gsj;
            R = s_near[L];
        } else { // uniform: every thread read the same slots
            if (tid == 0) a.status[job.group] = 1;
            return;
        }
    }
}

hipError_t launch_group_upgma(const GroupUpgmaArgs& a, hipStream_t stream)
{
    if (a.n_jobs <= 0) return hipSuccess;
    if (a.max_m < 2 || a.max_m > UPGMA_GROUP_MAX_MEMBERS) return hipErrorInvalidValue;
    if (a.total_rows <= 0 || a.total_rows > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upgma_group_dist_kernel, dim3((unsigned)a.total_rows), dim3(256), 0, stream, a);
    // four waves up to 1024 members, sixteen beyond: where mst_group_prim_kernel switches (a barrier over four waves is
    // the shortest; beyond 1024 members a thread would own more than four rows)
    const dim3 grid((unsigned)a.n_jobs);
    const bool wide = a.max_m > 1024;
#define GROUP_UPGMA(M, T) \
    hipLaunchKernelGGL((upgma_group_kernel<M, T>), grid, dim3(T), group_upgma_lds_bytes(T, a.max_m), stream, a)
    if (a.modified) {
        if (!wide) GROUP_UPGMA(true, 256); else GROUP_UPGMA(true, 1024);
    } else {
        if (!wide) GROUP_UPGMA(false, 256); else GROUP_UPGMA(false, 1024);
    }
#undef GROUP_UPGMA
    return hipGetLastError();
}

} // namespace lcsgpu
