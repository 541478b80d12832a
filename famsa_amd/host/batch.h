// batch.h -- guide trees for many FASTA files in one process, on ONE engine context.
// A process that starts HIP pays 0.14-0.31 s before it computes anything, and a family of a few hundred sequences is
// all launch latency to the one-file path (eight Boruvka rounds of five or more launches each, one busy CU).  Here the
// files are loaded and sorted on the host's worker threads, packed into CHUNKS, and a chunk's trees are made together:
// one upload of the chunk's records, then one lcsgpu_mst_prim_batch (-gt sl / slink: a workgroup per file), one
// lcsgpu_upgma_batch (-gt upgma / upgma_modified) or one lcsgpu_nj_batch (-gt nj): the merges of a file in a workgroup of
// its own.  FAMSA_HOST_TEST=batch_upgma_host / batch_nj_host send those files' triangles (lcsgpu_lcs_triangles_batch) to the
// host builders on the worker threads instead, as does a -gt nj file above LCSGPU_NJ_BATCH_MAX_MEMBERS (with the routing
// limit lifted).
// Every file's Newick is what guide_tree_newick_gpu gives for it alone: the same guide_tree_newick runs over a view of
// the file's slice of the chunk.  Files the chunks do not take -- more unique sequences than the routing limit, a
// sequence beyond 65535 residues, a tree heuristic that applies, -gt chained, -gt sl with an orientation-sensitive
// member -- go through the one-file path on the same engine afterwards.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "pipeline.h"

namespace famsa_host {

struct BatchJob {
    std::string input; // FASTA path
    TreeOptions opt;
};
struct BatchResult {
    bool ok = false;
    std::string newick;  // ok
    std::string message; // !ok: what went wrong with THIS file (the others are still made)
    int route = -1;      // 0 = in a chunk, 1 = the one-file path, -1 = failed before it had one
};
struct BatchTotals {
    int files = 0, chunks = 0, in_chunks = 0, one_file = 0, failed = 0;
    int device_upgma = 0; // files of the chunks whose UPGMA merges ran on the device (lcsgpu_upgma_batch)
    int device_nj = 0;    // ... whose NJ merges did (lcsgpu_nj_batch)
    // load / sort / newick: summed over the worker threads; upload / device: the driving thread's wall time
    double load_s = 0, sort_s = 0, upload_s = 0, device_s = 0, newick_s = 0, one_file_s = 0;
};

// The chunk planner (pure): files in order; file i goes into a chunk only if eligible[i] and unique_counts[i] <= group_max;
// consecutive such files share a chunk while the chunk's sum of m (m - 1) / 2 stays within pair_budget (a file that
// does not fit opens the next chunk; a file larger than the whole budget gets a chunk to itself).  chunk_of[i] = the
// chunk's number, -1 = the one-file route.  Returns the number of chunks.
int batch_plan(const std::vector<int64_t>& unique_counts, const std::vector<uint8_t>& eligible, int64_t pair_budget, int group_max,
               std::vector<int>& chunk_of);
// the defaults (FAMSA_HOST_TEST batch_pairs=N / batch_group_max=N override them: tests)
int64_t batch_pair_budget();
int batch_group_max();

// One Newick per job.  done(i, result), when given, is called as soon as file i is finished -- from a worker thread or
// the driving one, never for the same i twice -- so that a caller can store results while later chunks are computed.
// devices[0] only.  An engine that cannot be created fails every file with the same message.
std::vector<BatchResult> guide_trees_newick_gpu(const std::vector<BatchJob>& jobs, int device, BatchTotals* totals = nullptr,
                                                EngineFuture* engine = nullptr,
                                                const std::function<void(size_t, const BatchResult&)>& done = nullptr);

} // namespace famsa_host
