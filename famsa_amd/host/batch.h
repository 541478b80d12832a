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
// dist_exports_gpu does the same for distance matrices (-dist_export): the same workers, packer, engine and failure
// isolation; a chunk is one upload and one lcsgpu_dist_text_batch, and the workers write its files.
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
// -dist_export of one file of a batch: the matrix of `input`'s records, as read, written to `output`
struct DistJob {
    std::string input, output;
    Distance dist = Distance::indel075_div_lcs;
    bool square = false, pid = false;
    int n_threads = 1; // host worker threads of the batch (the smallest of the jobs')
};
struct BatchTotals {
    int files = 0, chunks = 0, in_chunks = 0, one_file = 0, failed = 0;
    int device_upgma = 0; // files of the chunks whose UPGMA merges ran on the device (lcsgpu_upgma_batch)
    int device_nj = 0;    // ... whose NJ merges did (lcsgpu_nj_batch)
    // load / sort / newick: summed over the worker threads; upload / device: the driving thread's wall time
    double load_s = 0, sort_s = 0, upload_s = 0, device_s = 0, newick_s = 0, one_file_s = 0;
    // dist_exports_gpu: the bytes of the chunks' texts; kernel_s = the part of device_s (the chunks' calls) between the first
    // LCS launch and the end of the write pass by the device's clock -- the rest is the call's planning and the text's copy
    // to the host --, store_s = the writes of the files, summed over the worker threads
    uint64_t text_bytes = 0;
    double kernel_s = 0, store_s = 0;
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
// the matrices' chunks (dist_exports_gpu): values per chunk -- batch_pair_budget(), but at most 2^22 (FAMSA_HOST_TEST
// batch_values=N: another cap, measurements)
int64_t batch_value_budget();

// One Newick per job.  done(i, result), when given, is called as soon as file i is finished -- from a worker thread or
// the driving one, never for the same i twice -- so that a caller can store results while later chunks are computed.
// devices[0] only.  An engine that cannot be created fails every file with the same message.
std::vector<BatchResult> guide_trees_newick_gpu(const std::vector<BatchJob>& jobs, int device, BatchTotals* totals = nullptr,
                                                EngineFuture* engine = nullptr,
                                                const std::function<void(size_t, const BatchResult&)>& done = nullptr);

// -dist_export [-pid] [-square_matrix] for many files on one engine context: every output is what dist_export_gpu writes for
// that input alone.  A file's records stay in input order, duplicates included (the set as it was read).  Files of at most
// batch_group_max() records without a sequence beyond 65535 residues are packed into chunks by their VALUES -- m (m - 1) / 2,
// m^2 with square -- against batch_value_budget(); a chunk is one upload and one lcsgpu_dist_text_batch, whose text the worker
// threads put into the files (the -square_matrix header first) while the driving thread goes on with the next chunk: the
// call keeps two text buffers, so chunk k's writers are waited for before the call of chunk k + 2.  The other files, and all
// files of a chunk whose text does not fit (LCSGPU_E_NOMEM), go through write_distance_csv on the same engine afterwards.
// A file that fails (unreadable or empty input, an output that cannot be opened or written) fails alone.  Consecutive jobs
// with the same (dist, square, pid) share chunks.  done as for guide_trees_newick_gpu; BatchResult::newick stays empty.
std::vector<BatchResult> dist_exports_gpu(const std::vector<DistJob>& jobs, int device, BatchTotals* totals = nullptr,
                                          EngineFuture* engine = nullptr,
                                          const std::function<void(size_t, const BatchResult&)>& done = nullptr);

} // namespace famsa_host
