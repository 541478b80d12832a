#include "batch.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <future>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "../../include/lcsgpu.h"

namespace famsa_host {

namespace {

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The planner's step, shared by batch_plan and the driver (which learns the unique counts file by file, in order).
struct ChunkPacker {
    int64_t budget;
    int group_max;
    int chunk = -1;
    int64_t used = 0;
    int place(int64_t m, bool eligible) { return place(m, m > 1 ? m * (m - 1) / 2 : 0, eligible); }
    // ... with what the file takes of the budget given by the caller (the matrices of -dist_export: their values)
    int place(int64_t m, int64_t cost, bool eligible)
    {
        if (!eligible || m > group_max) return -1;
        if (chunk < 0 || used + cost > budget) {
            ++chunk;
            used = 0;
        }
        used += cost;
        return chunk;
    }
};

// worker threads of the batch: loading + sorting files, and turning a chunk's device results into Newick texts
class Pool {
public:
    explicit Pool(int n_threads)
    {
        for (int t = 0; t < std::max(1, n_threads); ++t) threads_.emplace_back([this] { work(); });
    }
    ~Pool()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    void submit(std::function<void()> task)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            tasks_.push_back(std::move(task));
            ++pending_;
        }
        cv_.notify_one();
    }
    void wait_idle()
    {
        std::unique_lock<std::mutex> lk(mu_);
        idle_.wait(lk, [this] { return pending_ == 0; });
    }

private:
    void work()
    {
        for (;;) {
            std::function<void()> task;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return stop_ || !tasks_.empty(); });
                if (tasks_.empty()) return;
                task = std::move(tasks_.front());
                tasks_.pop_front();
            }
            task(); // (tasks catch what they throw)
            {
                std::lock_guard<std::mutex> lk(mu_);
                --pending_;
            }
            idle_.notify_all();
        }
    }
    std::vector<std::thread> threads_;
    std::deque<std::function<void()>> tasks_;
    std::mutex mu_;
    std::condition_variable cv_, idle_;
    int pending_ = 0;
    bool stop_ = false;
};

// A file's slice of a chunk as the tree builders see it: ids 0 .. m - 1 = the file's sorted unique working order.  Prim's
// edges come from the chunk's lcsgpu_mst_prim_batch, UPGMA's node records from its lcsgpu_upgma_batch, NJ's from its
// lcsgpu_nj_batch, the triangle from its lcsgpu_lcs_triangles_batch; nothing is computed here.
class SliceLcsSource : public LcsSource {
public:
    SliceLcsSource(const SeqSet& s, const std::vector<int>& in_of, bool sensitive) : s_(s), in_of_(in_of), sensitive_(sensitive) {}
    const uint16_t* tri = nullptr;   // the slice's packed triangle, or NULL
    const MstEdge* edges = nullptr;  // its m - 1 MST records, or NULL
    int edges_kind = -1;
    bool edges_triangle_orientation = false;
    const int32_t* left = nullptr;   // its m - 1 UPGMA or NJ node records, or NULL
    const int32_t* right = nullptr;
    int nodes_kind = -1;
    bool nodes_modified = false;
    bool nodes_nj = false;           // the records are neighbour joining's
    bool nodes_failed = false;       // the device found no finite nearest neighbour (UPGMA) / no finite q (NJ) in this file

    int n() const override { return (int)in_of_.size(); }
    uint32_t length(int i) const override { return s_.length((size_t)in_of_[(size_t)i]); }
    bool orientation_sensitive() const override { return sensitive_; }
    bool wide() const override { return false; } // (a chunk takes no file with a sequence beyond 65535 residues)
    bool whole_input() const override { return true; }
    const void* triangle_view() const override { return tri; }
    void triangle(int r0, int r1, LcsBuf& out) override
    {
        if (!tri) throw std::runtime_error("batch: the chunk holds no LCS triangle for this file");
        const size_t a = (size_t)r0 * (r0 > 0 ? r0 - 1 : 0) / 2, b = (size_t)r1 * (r1 > 0 ? r1 - 1 : 0) / 2;
        out.resize(b - a, false);
        std::copy(tri + a, tri + b, out.v16.begin());
    }
    void rect(const int*, int, const int*, int, LcsBuf&) override
    {
        throw std::runtime_error("batch: a chunk serves triangles and MST records only");
    }
    bool prim_edges(int distance_kind, std::vector<MstEdge>& out, bool triangle_orientation) override
    {
        if (!edges || distance_kind != edges_kind || triangle_orientation != edges_triangle_orientation) return false;
        out.assign(edges, edges + (n() > 0 ? n() - 1 : 0));
        return true;
    }
    bool upgma_nodes(int distance_kind, bool modified, std::vector<int32_t>& l, std::vector<int32_t>& r) override
    {
        if (!left || !right || nodes_nj || distance_kind != nodes_kind || modified != nodes_modified) return false;
        if (nodes_failed) // what the host builder says for such a file (trees.cpp)
            throw std::runtime_error("UPGMA: no finite nearest neighbour (a pair with LCS 0?) -- the reference's "
                                     "algorithm is undefined for this input");
        l.assign(left, left + (n() > 0 ? n() - 1 : 0));
        r.assign(right, right + (n() > 0 ? n() - 1 : 0));
        return true;
    }
    bool nj_nodes(int distance_kind, std::vector<int32_t>& l, std::vector<int32_t>& r) override
    {
        if (!left || !right || !nodes_nj || distance_kind != nodes_kind) return false;
        if (nodes_failed) // what the host builder says for such a file (trees.cpp, nj_tree)
            throw std::runtime_error("NJ: no finite q (a pair with LCS 0?) -- the reference's result is degenerate for this input");
        l.assign(left, left + (n() > 0 ? n() - 1 : 0));
        r.assign(right, right + (n() > 0 ? n() - 1 : 0));
        return true;
    }

private:
    const SeqSet& s_;
    const std::vector<int>& in_of_;
    bool sensitive_;
};

struct Loaded {
    SeqSet s;
    WorkSet w;
    std::vector<int> in_of; // unique index -> record of the file
    bool ok = false, eligible = false;
    std::string message;
};

bool is_mst(GT m) { return m == GT::MST_Prim || m == GT::SLINK; }
bool is_upgma(GT m) { return m == GT::UPGMA || m == GT::UPGMA_modified; }

} // namespace

int64_t batch_pair_budget()
{
    // 2 GiB of uint16 values: what the batched rectangles of the seed assignment take per launch (assign_batch_kb)
    return (int64_t)std::max(1, host_test_int("batch_pairs", 1 << 30));
}

int64_t batch_value_budget()
{
    // A value is ~9 B of text that the workers have to put into files, and a chunk's files are written while the NEXT chunk is
    // computed: chunks of 4 x 10^6 values (~38 MB of text) against one chunk for everything (profiles/batch_dist.txt, files per
    // second, medians of alternating runs): 430 against 220 at 1000 members, where the writes are most of the time (264
    // against 192 in an earlier run); 2092 against 2203 and 2629 against 2035 at 200 and 50, both inside each other's
    // run-to-run range.
    return std::min<int64_t>(batch_pair_budget(), std::max(1, host_test_int("batch_values", 1 << 22)));
}

int batch_group_max()
{
    // The largest measured family size at which the chunks are ahead of both the one-file route on the same context and a
    // guide_tree loop, for -gt sl and for -gt upgma (profiles/batch_trees.txt: 849 / 316 files/s against 322 / 169 and 51 / 51
    // at 1000 members; at 4000 -gt upgma gained nothing while its merges ran in the host builders -- with a workgroup per file
    // it does, 59-63 against 24-28 files/s, profiles/batch_upgma.txt: the case for a limit per method, not taken yet); never
    // above LCSGPU_MST_BATCH_MAX_MEMBERS.
    return std::max(0, std::min(4096, host_test_int("batch_group_max", 1000)));
}

int batch_plan(const std::vector<int64_t>& unique_counts, const std::vector<uint8_t>& eligible, int64_t pair_budget, int group_max,
               std::vector<int>& chunk_of)
{
    ChunkPacker packer{pair_budget, std::min(group_max, 4096)};
    chunk_of.assign(unique_counts.size(), -1);
    for (size_t i = 0; i < unique_counts.size(); ++i) chunk_of[i] = packer.place(unique_counts[i], i < eligible.size() && eligible[i] != 0);
    return packer.chunk + 1;
}

namespace {

// What the batches share (guide trees, distance matrices): the files' results and totals, failure isolation, the worker pool
// that loads files ahead of the device, the one engine, and the walk over the files in order -- chunk by chunk, then the
// one-file route.
class Driver {
public:
    using Done = std::function<void(size_t, const BatchResult&)>;
    Driver(size_t n_files, int n_threads, int device, EngineFuture* engine, const Done& done)
        : n(n_files), results(n_files), loaded(n_files), load_done_(n_files), done_(done), engine_(engine), pool(std::max(1, n_threads))
    {
        tot.files = (int)n;
        if (!engine_ && n > 0) {
            own_ = start_engine(device); // HIP initialisation runs beside the first loads
            engine_ = &own_;
        }
    }
    void finish(size_t i, BatchResult&& r)
    {
        results[i] = std::move(r);
        if (done_) done_(i, results[i]);
    }
    void fail_file(size_t i, const std::string& why, int route)
    {
        BatchResult r;
        r.message = why;
        r.route = route;
        {
            std::lock_guard<std::mutex> lk(tot_mu);
            ++tot.failed;
        }
        finish(i, std::move(r));
    }
    GpuLcsSource* the_engine()
    {
        if (!held_ && engine_error.empty()) {
            try {
                held_ = engine_->get();
            } catch (const std::exception& e) {
                engine_error = e.what();
            }
        }
        return held_.get();
    }
    // load_one(i, f) fills f (on a worker; what it throws is the file's message); place(i) = the file's chunk number or -1;
    // run_chunk(files) when a chunk is full; then one_file_route(i, engine) for one_file, in list order
    void run(const std::function<void(size_t, Loaded&)>& load_one, const std::function<int(size_t)>& place,
             const std::function<void(const std::vector<size_t>&)>& run_chunk, const std::function<void(size_t, GpuLcsSource&)>& one_file_route)
    {
        size_t submitted = 0;
        const size_t lookahead = 256; // files loaded ahead of the chunk the device works on
        auto submit_loads = [&](size_t upto) {
            for (; submitted < std::min(n, upto); ++submitted) {
                const size_t i = submitted;
                auto pr = std::make_shared<std::promise<void>>();
                load_done_[i] = pr->get_future();
                pool.submit([this, &load_one, i, pr] {
                    auto f = std::make_shared<Loaded>();
                    try {
                        load_one(i, *f);
                        f->ok = true;
                    } catch (const std::exception& e) {
                        f->message = e.what();
                    }
                    loaded[i] = f;
                    pr->set_value();
                });
            }
        };
        std::vector<size_t> current;
        int current_chunk = -1;
        for (size_t i = 0; i < n; ++i) {
            submit_loads(i + lookahead);
            load_done_[i].get();
            const Loaded& f = *loaded[i];
            if (!f.ok) {
                fail_file(i, f.message, -1);
                loaded[i].reset();
                continue;
            }
            const int c = place(i);
            if (c < 0) {
                one_file.push_back(i);
                continue;
            }
            if (c != current_chunk && !current.empty()) { // the chunk is full: the device takes it while the workers load on
                run_chunk(current);
                current.clear();
            }
            current_chunk = c;
            current.push_back(i);
        }
        if (!current.empty()) run_chunk(current);

        // everything else: today's one-file path, one after the other, on the same engine
        std::sort(one_file.begin(), one_file.end());
        for (size_t i : one_file) {
            GpuLcsSource* src = the_engine();
            if (!src) {
                fail_file(i, engine_error, 1);
                continue;
            }
            try {
                one_file_route(i, *src);
            } catch (const std::exception& e) {
                fail_file(i, e.what(), 1);
            }
            loaded[i].reset();
        }
        pool.wait_idle();
        if (g_abandon_engine_at_return && !profile_on()) (void)held_.release();
    }

    const size_t n;
    std::vector<BatchResult> results;
    BatchTotals tot;
    std::mutex tot_mu; // the totals the workers add to
    std::vector<std::shared_ptr<Loaded>> loaded;
    std::string engine_error;
    std::vector<size_t> one_file; // in list order; a chunk may add files it cannot serve

private:
    std::vector<std::future<void>> load_done_;
    Done done_;
    EngineFuture own_, *engine_;
    std::unique_ptr<GpuLcsSource> held_;

public:
    Pool pool; // (the last member: its threads end before anything they use does)
};

} // namespace

std::vector<BatchResult> guide_trees_newick_gpu(const std::vector<BatchJob>& jobs, int device, BatchTotals* totals, EngineFuture* engine,
                                                const std::function<void(size_t, const BatchResult&)>& done)
{
    const size_t n = jobs.size();
    if (n == 0) {
        BatchTotals none;
        if (totals) *totals = none;
        return {};
    }
    int n_threads = jobs[0].opt.fast.n_threads;
    for (const auto& j : jobs) n_threads = std::min(n_threads, j.opt.fast.n_threads);
    Driver d(n, n_threads, device, engine, done);
    BatchTotals& tot = d.tot;
    std::mutex& tot_mu = d.tot_mu;
    std::vector<std::shared_ptr<Loaded>>& loaded = d.loaded;
    Pool& pool = d.pool;
    std::vector<size_t>& one_file = d.one_file; // the chunks add the -gt sl files they find an orientation-sensitive member in
    auto finish = [&](size_t i, BatchResult&& r) { d.finish(i, std::move(r)); };
    auto fail_file = [&](size_t i, const std::string& why, int route) { d.fail_file(i, why, route); };

    auto load_one = [&](size_t i, Loaded& ld) {
        Loaded* f = &ld;
        const TreeOptions& opt = jobs[i].opt;
        const double t0 = now_s();
        f->s = load_fasta(jobs[i].input, 1);
        if (f->s.size() == 0) throw std::runtime_error("no sequences in " + jobs[i].input);
        const double t1 = now_s();
        f->w = make_workset(f->s, opt.keep_duplicates, 1);
        f->in_of.resize((size_t)f->w.n_unique());
        for (int a = 0; a < f->w.n_unique(); ++a) f->in_of[(size_t)a] = f->w.sorted2input[(size_t)f->w.unique2sorted[(size_t)a]];
        uint32_t longest = 0;
        for (size_t r = 0; r < f->s.size(); ++r) longest = std::max(longest, f->s.length(r));
        // what guide_tree_newick decides for the file alone: a heuristic applies from the threshold on (all records count)
        const bool heuristic = opt.heuristic != 0 && (int)f->s.size() >= opt.fast.threshold;
        f->eligible = longest <= 65535 && !heuristic && opt.method != GT::chained &&
                      (opt.dist == Distance::indel_div_lcs || opt.dist == Distance::indel075_div_lcs);
        const double t2 = now_s();
        std::lock_guard<std::mutex> lk(tot_mu);
        tot.load_s += t1 - t0;
        tot.sort_s += t2 - t1;
    };

    // what a chunk's device calls leave behind for the workers
    struct ChunkData {
        std::vector<LcsSource::MstEdge> edges[4]; // by (triangle orientation, distance kind)
        LcsBuf tri;
        std::vector<int32_t> left[6], right[6], status[6]; // UPGMA by (modified, distance kind), then NJ by distance kind
    };
    auto run_chunk = [&](const std::vector<size_t>& files) {
        GpuLcsSource* src = d.the_engine();
        if (!src) {
            for (size_t i : files) fail_file(i, d.engine_error, 0);
            return;
        }
        std::vector<size_t> pending = files; // not finished yet: what an error of the chunk's calls fails
        try {
            const double t0 = now_s();
            // the chunk's records, file after file as they were read; ids = every file's sorted unique order, one after the other
            size_t n_records = 0, n_codes = 0, n_ids = 0;
            for (size_t i : files) {
                n_records += loaded[i]->s.size();
                n_codes += loaded[i]->s.codes.size();
                n_ids += loaded[i]->in_of.size();
            }
            if (n_records > 0x7fffffffu || n_ids > 0x7fffffffu) throw std::runtime_error("batch: a chunk of more than 2^31 records");
            Bytes codes(n_codes);
            std::vector<uint64_t> offsets;
            offsets.reserve(n_records + 1);
            std::vector<int> order;
            order.reserve(n_ids);
            std::vector<int> id0(files.size());
            size_t code_at = 0, rec_at = 0;
            for (size_t k = 0; k < files.size(); ++k) {
                const Loaded& f = *loaded[files[k]];
                std::copy(f.s.codes.begin(), f.s.codes.end(), codes.begin() + (ptrdiff_t)code_at);
                for (size_t r = 0; r < f.s.size(); ++r) offsets.push_back(f.s.offsets[r] + code_at);
                id0[k] = (int)order.size();
                for (int rec : f.in_of) order.push_back((int)rec_at + rec);
                code_at += f.s.codes.size();
                rec_at += f.s.size();
            }
            offsets.push_back(code_at);
            src->upload_ordered(codes.data(), offsets, order);
            const std::vector<uint8_t>& flags = src->orientation_flags();
            const double t1 = now_s();

            auto data = std::make_shared<ChunkData>();
            std::vector<char> sensitive(files.size(), 0);
            // which of the eleven requests serves the file: 0 .. 3 = Prim's edges, 4 = the triangles, 5 .. 8 = UPGMA's node
            // records, 9 .. 10 = NJ's
            std::vector<int> list_of(files.size(), -1);
            std::vector<size_t> at(files.size(), 0);        // where its records / its triangle start in that request's result
            std::vector<int> group_of(files.size(), 0);     // its list number inside the request
            std::vector<std::vector<int>> ids(11);
            std::vector<std::vector<int64_t>> offs(11, std::vector<int64_t>{0});
            std::vector<size_t> filled(11, 0);
            const bool upgma_on_host = host_test("batch_upgma_host"), nj_on_host = host_test("batch_nj_host");
            for (size_t k = 0; k < files.size(); ++k) {
                const size_t i = files[k];
                const Loaded& f = *loaded[i];
                const TreeOptions& opt = jobs[i].opt;
                const int m = (int)f.in_of.size();
                for (int a = 0; a < m; ++a) sensitive[k] |= flags[(size_t)(id0[k] + a)] != 0;
                if (m < 2) continue; // one unique sequence: no tree stage (guide_tree_newick)
                int list;
                if (opt.method == GT::MST_Prim && sensitive[k]) { // MSTPrim wants LCS(ref = the node just added): not in a triangle
                    one_file.push_back(i);
                    pending.erase(std::find(pending.begin(), pending.end(), i));
                    list_of[k] = -2;
                    continue;
                }
                if (is_mst(opt.method)) list = (opt.method == GT::SLINK ? 2 : 0) + (opt.dist == Distance::indel075_div_lcs ? 1 : 0);
                else if (is_upgma(opt.method) && !upgma_on_host)
                    list = 5 + (opt.method == GT::UPGMA_modified ? 2 : 0) + (opt.dist == Distance::indel075_div_lcs ? 1 : 0);
                // -gt nj: every size a chunk takes goes to the device.  Files per second against the host builders of the commit
                // before, in alternating runs (profiles/batch_nj.txt): 3119 against 2011 at 50 members, 1339 against 1036 at
                // 200, 280 against 59 at 1000 -- no size is behind, so there is no lower threshold.
                else if (opt.method == GT::NJ && !nj_on_host && m <= LCSGPU_NJ_BATCH_MAX_MEMBERS) // (above: the routing limit was lifted)
                    list = 9 + (opt.dist == Distance::indel075_div_lcs ? 1 : 0);
                else list = 4;
                list_of[k] = list;
                group_of[k] = (int)offs[(size_t)list].size() - 1;
                at[k] = filled[(size_t)list];
                filled[(size_t)list] += list == 4 ? (size_t)m * (m - 1) / 2 : (size_t)(m - 1);
                for (int a = 0; a < m; ++a) ids[(size_t)list].push_back(id0[k] + a);
                offs[(size_t)list].push_back((int64_t)ids[(size_t)list].size());
            }
            for (int list = 0; list < 4; ++list)
                if (offs[(size_t)list].size() > 1)
                    src->prim_edges_batch(ids[(size_t)list].data(), offs[(size_t)list].data(), (int)offs[(size_t)list].size() - 1, list & 1,
                                          list >= 2, data->edges[list]);
            if (offs[4].size() > 1) src->triangles_batch(ids[4].data(), offs[4].data(), (int)offs[4].size() - 1, data->tri);
            for (int list = 5; list < 9; ++list)
                if (offs[(size_t)list].size() > 1)
                    src->upgma_nodes_batch(ids[(size_t)list].data(), offs[(size_t)list].data(), (int)offs[(size_t)list].size() - 1,
                                           (list - 5) & 1, list >= 7, data->left[list - 5], data->right[list - 5], data->status[list - 5]);
            for (int list = 9; list < 11; ++list)
                if (offs[(size_t)list].size() > 1)
                    src->nj_nodes_batch(ids[(size_t)list].data(), offs[(size_t)list].data(), (int)offs[(size_t)list].size() - 1, list - 9,
                                        data->left[list - 5], data->right[list - 5], data->status[list - 5]);
            const double t2 = now_s();
            {
                std::lock_guard<std::mutex> lk(tot_mu);
                tot.upload_s += t1 - t0;
                tot.device_s += t2 - t1;
                ++tot.chunks;
            }
            // the conversions of the chunk's files, on the workers; the next chunk's upload does not touch what they read
            for (size_t k = 0; k < files.size(); ++k) {
                if (list_of[k] == -2) continue;
                const size_t i = files[k];
                const int list = list_of[k];
                const size_t where = at[k];
                const bool sens = sensitive[k] != 0;
                const int group = group_of[k];
                pool.submit([&, i, list, where, group, sens, data] {
                    std::shared_ptr<Loaded> f = loaded[i];
                    try {
                        const double c0 = now_s();
                        SliceLcsSource view(f->s, f->in_of, sens);
                        if (list == 4) view.tri = data->tri.v16.data() + where;
                        else if (list >= 5) {
                            view.left = data->left[list - 5].data() + where;
                            view.right = data->right[list - 5].data() + where;
                            view.nodes_kind = (list - 5) & 1;
                            view.nodes_modified = list == 7 || list == 8;
                            view.nodes_nj = list >= 9;
                            view.nodes_failed = data->status[list - 5][(size_t)group] != 0;
                        } else if (list >= 0) {
                            view.edges = data->edges[list].data() + where;
                            view.edges_kind = list & 1;
                            view.edges_triangle_orientation = list >= 2;
                        }
                        BatchResult r;
                        r.newick = guide_tree_newick(f->s, f->w, view, jobs[i].opt);
                        r.ok = true;
                        r.route = 0;
                        {
                            std::lock_guard<std::mutex> lk(tot_mu);
                            tot.newick_s += now_s() - c0;
                            ++tot.in_chunks;
                            if (list >= 9) ++tot.device_nj;
                            else if (list >= 5) ++tot.device_upgma;
                        }
                        finish(i, std::move(r));
                    } catch (const std::exception& e) {
                        fail_file(i, e.what(), 0);
                    }
                    loaded[i].reset();
                });
            }
        } catch (const std::exception& e) {
            for (size_t i : pending) fail_file(i, e.what(), 0);
        }
    };

    ChunkPacker packer{batch_pair_budget(), batch_group_max()};
    d.run(load_one, [&](size_t i) { return packer.place(loaded[i]->w.n_unique(), loaded[i]->eligible); }, run_chunk,
          [&](size_t i, GpuLcsSource& src) {
              const double t0 = now_s();
              BatchResult r;
              r.newick = guide_tree_newick_gpu(loaded[i]->s, src, jobs[i].opt, nullptr);
              r.ok = true;
              r.route = 1;
              {
                  std::lock_guard<std::mutex> lk(tot_mu);
                  tot.one_file_s += now_s() - t0;
                  ++tot.one_file;
              }
              finish(i, std::move(r));
          });
    if (totals) *totals = tot;
    return std::move(d.results);
}

namespace {

// header (may be empty) + text into a fresh file; what goes wrong, in the one-file path's words
void write_csv_file(const std::string& path, const std::string& header, const char* text, uint64_t bytes)
{
    const int fd = open(path.c_str(), O_CREAT | O_TRUNC | O_WRONLY | O_CLOEXEC, 0666);
    if (fd < 0) throw std::runtime_error("cannot open " + path);
    auto put = [&](const char* p, uint64_t len) {
        while (len) {
            const ssize_t k = write(fd, p, (size_t)std::min<uint64_t>(len, (uint64_t)1 << 30));
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) return false;
            p += k;
            len -= (uint64_t)k;
        }
        return true;
    };
    const bool ok = put(header.data(), header.size()) && put(text, bytes);
    if (close(fd) != 0 || !ok) throw std::runtime_error("writing " + path + " failed (disk full?)");
}

// the writers of one chunk: the chunk after the next may not be computed before they are through (the text buffer is theirs)
struct WriteWave {
    std::mutex mu;
    std::condition_variable cv;
    size_t left = 0;
    void done()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            --left;
        }
        cv.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return left == 0; });
    }
};

} // namespace

std::vector<BatchResult> dist_exports_gpu(const std::vector<DistJob>& jobs, int device, BatchTotals* totals, EngineFuture* engine,
                                          const std::function<void(size_t, const BatchResult&)>& done)
{
    const size_t n = jobs.size();
    if (n == 0) {
        BatchTotals none;
        if (totals) *totals = none;
        return {};
    }
    int n_threads = jobs[0].n_threads;
    for (const auto& j : jobs) n_threads = std::min(n_threads, j.n_threads);
    Driver d(n, n_threads, device, engine, done);
    auto same_mode = [&](size_t a, size_t b) { return jobs[a].dist == jobs[b].dist && jobs[a].square == jobs[b].square && jobs[a].pid == jobs[b].pid; };
    auto made = [&](size_t i, int route) {
        BatchResult r;
        r.ok = true;
        r.route = route;
        d.finish(i, std::move(r));
    };

    auto load_one = [&](size_t i, Loaded& f) {
        const double t0 = now_s();
        f.s = load_fasta(jobs[i].input, 1);
        if (f.s.size() == 0) throw std::runtime_error("no sequences in " + jobs[i].input);
        uint32_t longest = 0;
        for (size_t r = 0; r < f.s.size(); ++r) longest = std::max(longest, f.s.length(r));
        f.eligible = longest <= 65535; // all records count: no dedup, no tree heuristic
        std::lock_guard<std::mutex> lk(d.tot_mu);
        d.tot.load_s += now_s() - t0;
    };

    std::shared_ptr<WriteWave> waves[2]; // the writers of the last two chunks, by the text buffer they read
    int n_calls = 0;
    auto run_chunk = [&](const std::vector<size_t>& files) {
        GpuLcsSource* src = d.the_engine();
        if (!src) {
            for (size_t i : files) d.fail_file(i, d.engine_error, 0);
            return;
        }
        try {
            const double t0 = now_s();
            const DistJob& mode = jobs[files[0]];
            // the chunk's records, file after file as they were read: list k = the ids of file k, a contiguous range
            size_t n_records = 0, n_codes = 0, n_name_bytes = 0;
            for (size_t i : files) {
                n_records += d.loaded[i]->s.size();
                n_codes += d.loaded[i]->s.codes.size();
                for (const auto& id : d.loaded[i]->s.ids) n_name_bytes += id.size();
            }
            if (n_records > 0x7fffffffu) throw std::runtime_error("batch: a chunk of more than 2^31 records");
            Bytes codes(n_codes);
            std::vector<uint64_t> offsets, name_off;
            offsets.reserve(n_records + 1);
            name_off.reserve(n_records + 1);
            std::string names;
            names.reserve(n_name_bytes);
            std::vector<int> ids(n_records);
            std::vector<int64_t> list_off{0};
            size_t code_at = 0;
            for (size_t i : files) {
                const SeqSet& s = d.loaded[i]->s;
                std::copy(s.codes.begin(), s.codes.end(), codes.begin() + (ptrdiff_t)code_at);
                for (size_t r = 0; r < s.size(); ++r) {
                    offsets.push_back(s.offsets[r] + code_at);
                    name_off.push_back(names.size());
                    names.append(s.ids[r].c_str() + 1); // as the reference prints it: from the second character to the first NUL
                }
                code_at += s.codes.size();
                list_off.push_back((int64_t)offsets.size());
            }
            offsets.push_back(code_at);
            name_off.push_back(names.size());
            for (size_t k = 0; k < n_records; ++k) ids[k] = (int)k;
            src->upload(codes.data(), offsets); // input order, no sort, no dedup: the sets as they were read
            const double t1 = now_s();
            // the buffer this call's text comes in was the call before last's: its writers first
            std::shared_ptr<WriteWave>& wave = waves[n_calls & 1];
            if (wave) wave->wait();
            const char* text = nullptr;
            std::vector<uint64_t> text_off;
            const double t_call = now_s(), kernel_ms0 = src->kernel_ms_total();
            if (!src->dist_text_batch(names, name_off, ids.data(), list_off.data(), (int)files.size(), (int)mode.dist, mode.square, mode.pid, text,
                                      text_off)) { // the text does not fit: file by file
                d.one_file.insert(d.one_file.end(), files.begin(), files.end());
                return;
            }
            ++n_calls;
            const double t2 = now_s();
            wave = std::make_shared<WriteWave>();
            wave->left = files.size();
            {
                std::lock_guard<std::mutex> lk(d.tot_mu);
                d.tot.upload_s += t1 - t0;
                d.tot.device_s += t2 - t_call;
                d.tot.kernel_s += 1e-3 * (src->kernel_ms_total() - kernel_ms0);
                d.tot.text_bytes += text_off.back();
                ++d.tot.chunks;
            }
            for (size_t k = 0; k < files.size(); ++k) {
                const size_t i = files[k];
                const char* const rows = text + text_off[k];
                const uint64_t bytes = text_off[k + 1] - text_off[k];
                std::shared_ptr<WriteWave> w = wave;
                d.pool.submit([&, i, rows, bytes, w] {
                    try {
                        const double c0 = now_s();
                        std::string header;
                        if (jobs[i].square) { // as write_csv_text builds it
                            for (const auto& id : d.loaded[i]->s.ids) {
                                header += ',';
                                header += id.c_str() + 1;
                            }
                            header += '\n';
                        }
                        write_csv_file(jobs[i].output, header, rows, bytes);
                        {
                            std::lock_guard<std::mutex> lk(d.tot_mu);
                            d.tot.store_s += now_s() - c0;
                            ++d.tot.in_chunks;
                        }
                        made(i, 0);
                    } catch (const std::exception& e) {
                        d.fail_file(i, e.what(), 0);
                    }
                    d.loaded[i].reset();
                    w->done();
                });
            }
        } catch (const std::exception& e) {
            for (size_t i : files) d.fail_file(i, e.what(), 0);
        }
    };

    ChunkPacker packer{batch_value_budget(), batch_group_max()};
    int mode_breaks = 0; // a change of (dist, square, pid) closes the chunk
    size_t last_placed = n;
    d.run(load_one,
          [&](size_t i) {
              const int64_t m = (int64_t)d.loaded[i]->s.size();
              const int c = packer.place(m, jobs[i].square ? m * m : m * (m - 1) / 2, d.loaded[i]->eligible);
              if (c < 0) return -1;
              if (last_placed < n && !same_mode(last_placed, i)) ++mode_breaks;
              last_placed = i;
              return c + mode_breaks;
          },
          run_chunk,
          [&](size_t i, GpuLcsSource& src) {
              const double t0 = now_s();
              const SeqSet& s = d.loaded[i]->s;
              src.upload(s.codes.data(), s.offsets);
              write_distance_csv(src, s.ids, jobs[i].dist, jobs[i].square, jobs[i].pid, jobs[i].output);
              {
                  std::lock_guard<std::mutex> lk(d.tot_mu);
                  d.tot.one_file_s += now_s() - t0;
                  ++d.tot.one_file;
              }
              made(i, 1);
          });
    if (totals) *totals = d.tot;
    return std::move(d.results);
}

} // namespace famsa_host
