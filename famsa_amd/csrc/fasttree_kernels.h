// fasttree_kernels.h -- internal interface between lcsgpu_fasttree.hip and the kernels behind the batched calls of the
// FastTree recursion (tree_kernels.hip, clarans_kernels.hip): all splits of a level in one launch wave.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcs_kernels.h"

namespace lcsgpu {

// ---- seed assignment of several evaluations in one launch (tree_kernels.hip) ----
struct AssignPiece {
    int64_t out0;    // element offset of the piece's LCS rectangle (n_seeds rows of n_cols)
    int32_t col0;    // first column: position in the launch's concatenated column list
    int32_t n_cols;
    int32_t seed0;   // first seed: position in the concatenated seed list
    int32_t n_seeds;
};
hipError_t launch_assign_seeds_batch(const void* lcs, int elem_size, const AssignPiece* pieces, int32_t n_pieces, const int32_t* seed_ids,
                                     const int32_t* col_ids, int64_t n_cols, const uint32_t* lens, const float* pow_f32, int kind,
                                     float* dist, int32_t* assign, hipStream_t stream);

// ---- CLARANS for many samples at once: one workgroup runs a sample's whole chain of local searches (clarans_kernels.hip) ----
constexpr int CLARANS_STATE_WORDS = 32; // a chain's state block (ST_* in clarans_kernels.hip)
struct ClaransChain {
    ClaransArgs a;        // the search's buffers; a.draws / a.draws_len: the shape's pre-drawn step positions
    const int32_t* perm;  // [num_local][n_elems] before local search t, position i takes what position perm[t][i] held
    const int32_t* ids;   // [n_elems] the sample's sequence ids
    int32_t* best;        // [n_medoids] the medoids of the cheapest search so far
    int64_t tri0;         // element offset of the sample's packed LCS triangle in the launch's triangle buffer
    int32_t num_local;
    float* dn_member;     // [n_elems] by MEMBER: its distance to its medoid, 0 for a medoid (clarans_large_chain_kernel only)
};
// samples beyond CLARANS_MAX_MEDOIDS / CLARANS_MAX_NONMEDOIDS run in clarans_large_chain_kernel, up to this many members: the
// float matrix of a sample is 4.3 GB then, and (n - k) * k stays inside the reference's int (Clustering.cpp:21)
constexpr int CLARANS_LARGE_MAX_MEMBERS = 32768;
hipError_t launch_subset_distances_batch(const void* lcs, int elem_size, const ClaransChain* chains, int n_chains, int max_n,
                                         const uint32_t* lens, const float* pow_f32, int kind, hipStream_t stream);
// every chain in its own workgroup, to its end -- or until its pre-drawn positions run out, or for slice_us microseconds (0 = no limit)
hipError_t launch_clarans_chains(const ClaransChain* chains, int n_chains, int max_medoids, int slice_us, hipStream_t stream);
// the same for chains of any shape up to CLARANS_LARGE_MAX_MEMBERS (state in memory, walked in slices)
hipError_t launch_clarans_large_chains(const ClaransChain* chains, int n_chains, int slice_us, hipStream_t stream);

// ---- Prim's MST of many small groups in one launch: one workgroup per group (mst_kernels.hip) ----
constexpr int MST_GROUP_MAX_MEMBERS = 4096; // = LCSGPU_MST_BATCH_MAX_MEMBERS: a group's per-vertex state sits in one workgroup's LDS
struct GroupPrimJob {
    int64_t tri0;  // element offset of the group's packed LCS triangle in the launch's triangle buffer
    int64_t sq0;   // ... of its m x m square in the square buffer (square layout only)
    int64_t edge0; // record offset of its m - 1 edges
    int32_t id0;   // position of its first member in the concatenated id list
    int32_t m;     // members, 2 .. MST_GROUP_MAX_MEMBERS
};
struct GroupPrimArgs {
    const uint16_t* tri;      // the groups' packed triangles (ref = the later member)
    uint16_t* sq;             // NULL = read the triangles as they are; else the scratch the squares are expanded into
    const GroupPrimJob* jobs; // longest first
    const int64_t* row0;      // [n_jobs + 1] prefix sums of m over the jobs (the expansion's grid); square layout only
    const int32_t* ids;       // the concatenated id lists
    const uint32_t* lens;
    const double* pow_table;  // pow(i, 0.75), i < pow_n, from the host's libm
    MstEdge* edges;
    int64_t total_rows;       // row0[n_jobs]
    int32_t pow_n, n_jobs, kind, max_m;
};
hipError_t launch_group_prim(const GroupPrimArgs& a, hipStream_t stream);

// ---- UPGMA of many small groups: one workgroup per group (upgma_group_kernels.hip) ----
constexpr int UPGMA_GROUP_MAX_MEMBERS = MST_GROUP_MAX_MEMBERS; // = LCSGPU_UPGMA_BATCH_MAX_MEMBERS
struct GroupUpgmaJob {
    int64_t tri0;  // element offset of the group's packed LCS triangle in the launch's triangle buffer
    int64_t sq0;   // ... of its m x m float square in the launch's square buffer
    int64_t node0; // record offset of its m - 1 internal nodes
    int32_t id0;   // position of its first member in the concatenated id list
    int32_t m;     // members, 2 .. UPGMA_GROUP_MAX_MEMBERS
    int32_t group; // the caller's list number: where its status goes
    int32_t pad;
};
struct GroupUpgmaArgs {
    const uint16_t* tri;       // the groups' packed triangles (ref = the later member)
    float* sq;                 // the launch's squares
    const GroupUpgmaJob* jobs; // the launch's jobs, longest first
    const int64_t* row0;       // [n_jobs + 1] prefix sums of m over the launch's jobs
    const int32_t* ids;        // the concatenated id lists
    const uint32_t* lens;
    const float* pow_f32;      // (float) pow(i, 0.75)
    float* row_min;            // [total_rows] every row's initial key: distance,
    int32_t* row_near;         //              and column
    int32_t* left;
    int32_t* right;
    int32_t* status;           // [the call's groups] 1 = no finite nearest neighbour; zeroed before the launch
    int64_t total_rows;        // row0[n_jobs]
    int32_t n_jobs, kind, modified, max_m;
};
// the launch pair of a slice: the squares with the rows' initial keys, then the merges
hipError_t launch_group_upgma(const GroupUpgmaArgs& a, hipStream_t stream);

// ---- neighbour joining of many small groups: one workgroup per group (nj_group_kernels.hip) ----
constexpr int NJ_GROUP_MAX_MEMBERS = 2048; // = LCSGPU_NJ_BATCH_MAX_MEMBERS: a group costs m^3 / 6 evaluations of q on ONE CU
constexpr int NJ_GROUP_WIDE_AT = 200;      // groups from this many members on run in 1024 threads, smaller ones in 256 (profiles/batch_nj.txt)
struct GroupNjJob {
    int64_t tri0;  // element offset of the group's packed LCS triangle in the launch's triangle buffer
    int64_t f0;    // ... of its packed float triangle (same layout) in the launch's float buffer
    int64_t node0; // record offset of its m - 1 internal nodes
    int32_t id0;   // position of its first member in the concatenated id list
    int32_t m;     // members, 2 .. NJ_GROUP_MAX_MEMBERS
    int32_t group; // the caller's list number: where its status goes
    int32_t pad;
};
struct GroupNjArgs {
    const uint16_t* tri;    // the groups' packed triangles (ref = the later member)
    float* dist;            // the launch's float triangles
    const GroupNjJob* jobs; // the launch's jobs, longest first
    const int64_t* row0;    // [n_jobs + 1] prefix sums of m over the launch's jobs
    const int32_t* ids;     // the concatenated id lists
    const uint32_t* lens;
    const float* pow_f32;   // (float) pow(i, 0.75)
    float* row_sum;         // [total_rows] every row's initial sum of distances
    int32_t* left;
    int32_t* right;
    int32_t* status;        // [the call's groups] 1 = no q below FLT_MAX at some merge; zeroed before the launch
    int64_t total_rows;     // row0[n_jobs]
    int32_t n_jobs, kind, max_m;
    int32_t n_wide;         // the first n_wide jobs run in 1024 threads, the others in 256
    int32_t narrow_m;       // members of job n_wide, the longest of the others
};
// the launches of a slice: the float triangles with the rows' initial sums, then the merges
hipError_t launch_group_nj(const GroupNjArgs& a, hipStream_t stream);
// launches launch_group_nj makes for these arguments (the call's accounting)
int group_nj_launches(const GroupNjArgs& a);

} // namespace lcsgpu
