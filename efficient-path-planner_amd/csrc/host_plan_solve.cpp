// host_plan_solve.cpp — the batched solve of one planner attempt (plan_solve.h): the device
// stages in one launch each (plan_batch_launch), then per problem, on the planner threads,
// A* over its emitted rows (the row-restricted search, plan_geometry.h) or, when that cannot
// decide, over the whole k-NN table of its nodes.  The searches themselves: graph_search.h.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <iostream>
#include <mutex>
#include <thread>

#include <hip/hip_runtime_api.h>
#include <immintrin.h>

#include "completion.h"
#include "graph_search.h"
#include "host_scratch.h"
#include "plan_solve.h"

namespace epp {

namespace {
using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// Worker threads for PathPlanner::planPaths.  Grown on demand and never torn down (the
// process exit ends them; their thread-local device scratch is then left to the runtime
// rather than freed after it).
class PlanPool {
public:
    void submit(std::function<void()> job) {
        std::lock_guard<std::mutex> lk(mu_);
        q_.push_back(std::move(job));
        // a waiting thread per queued job, else one more thread
        if (idle_ < (int)q_.size()) std::thread([this] { loop(); }).detach();
        else cv_.notify_one();
    }

private:
    void loop() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            while (q_.empty()) {
                ++idle_;
                cv_.wait(lk);
                --idle_;
            }
            std::function<void()> job = std::move(q_.front());
            q_.pop_front();
            lk.unlock();
            job();
            lk.lock();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    int idle_ = 0;
};

PlanPool& plan_pool() {
    static PlanPool* pool = new PlanPool();  // intentionally leaked (see above)
    return *pool;
}

// Per calling thread: the batched planner's device workspace, pinned host block and stream
// (grown geometrically; freeing pinned memory synchronises the device).
class BatchScratch {
public:
    static BatchScratch& get() {
        thread_local BatchScratch b;
        return b;
    }
    static void regrow(void*& dev, size_t& cap, size_t bytes, const char* what) {
        if (dev) epp_free(dev);
        dev = nullptr;
        cap = 0;
        check(epp_malloc(&dev, bytes), what);
        cap = bytes;
    }
    void ensure(size_t dev_bytes, size_t host_bytes) {
        if (dev_bytes > dcap_) regrow(dev_, dcap_, std::max(dev_bytes, dcap_ + dcap_ / 2), "planner batch workspace");
        // (zeroed: the completion slots hold no stale sequence number)
        if (host_bytes > host_.cap &&
            host_.grow(std::max(host_bytes, host_.cap + host_.cap / 2), true) != hipSuccess)
            throw std::runtime_error("planner batch: hipHostMalloc failed");
    }
    void* dev() const { return dev_; }
    char* host() const { return host_.as<char>(); }
    uint32_t next_seq() { return epp::next_seq(seq_); }
    // Buffers of the whole-table search of one problem per planner thread (w), sized here
    // for n nodes: allocated with the batch, not on the planner threads when a search falls
    // back (a first allocation of pinned memory there took milliseconds).
    struct Area {
        void* dev = nullptr;
        PinnedBuf pin;
        void* stream = nullptr;
        size_t dcap = 0;
        bool cold = true;  // no whole-table search has run on it yet
    };
    static size_t r256(size_t b) { return (b + 255) & ~size_t(255); }
    // device: [edge counts | table (i32) | table (u16) | motion flags | k-NN workspace | the
    // reverse CSR: counts, fill, roff (n + 1), radj (i32), radj (u16)]; pinned: [edge counts
    // | nodes | table | roff | radj]
    static size_t area_dev_bytes(int64_t n, int k) {
        const size_t m = (size_t)n * k;
        return r256(16) + r256(m * 4) + r256(m * 2) + r256(m) + r256((size_t)epp_knn_workspace_size((int32_t)n)) +
               3 * r256((size_t)(n + 1) * 4) + r256(m * 4) + r256(m * 2);
    }
    static size_t area_pin_bytes(int64_t n, int k) {
        return r256(64) + r256((size_t)n * 24) + r256((size_t)n * k * 4) + r256((size_t)(n + 1) * 4) +
               r256((size_t)n * k * 4);
    }
    void ensure_areas(size_t W, int64_t n, int k) {
        if (areas_.size() < W) areas_.resize(W);
        const size_t db = area_dev_bytes(n, k), pb = area_pin_bytes(n, k);
        for (size_t w = 0; w < W; ++w) {
            Area& a = areas_[w];
            if (!a.stream) check(epp_stream_create(&a.stream), "stream");
            if (db > a.dcap) regrow(a.dev, a.dcap, db, "planner fallback workspace");
            if (pb > a.pin.cap) {
                if (a.pin.grow(pb) != hipSuccess) throw std::runtime_error("planner fallback: hipHostMalloc failed");
                // one DMA over the whole buffer now: the first transfers into fresh pinned
                // memory are slow (a first fallback took ~10 ms), and they belong here, with
                // the allocation (the cold first plan), not in a search
                check(epp_memcpy_d2h_async(a.pin.p, a.dev, std::min(pb, a.dcap), a.stream), "planner fallback warm-up");
                check(epp_stream_sync(a.stream), "planner fallback warm-up");
                // (cold stays as it was: a grown area -- a retry with doubled samples -- has
                // had its warm-up search; a new one starts cold)
            }
        }
    }
    Area& area(size_t w) { return areas_[w]; }
    void* stream() {
        if (!stream_) check(epp_stream_create(&stream_), "stream");
        return stream_;
    }
    ~BatchScratch() {
        if (dev_) epp_free(dev_);
        if (stream_) epp_stream_destroy(stream_);
        for (Area& a : areas_) {
            if (a.dev) epp_free(a.dev);
            if (a.stream) epp_stream_destroy(a.stream);
        }
    }

private:
    std::vector<Area> areas_;
    void* dev_ = nullptr;
    PinnedBuf host_;
    void* stream_ = nullptr;
    size_t dcap_ = 0;
    uint32_t seq_ = 0;
};

// A planner thread's buffers of its searches (grown with room to spare; warmed once per
// thread, before its first problem: a thread whose first problem came in a timed call paid
// the page faults there -- the second plan of a generator took ~2x).
struct SolveScratch {
    std::vector<double> ndc;      // the problem's referenced nodes (a private copy)
    std::vector<uint16_t> rowc;   // its rows (a private copy)
    std::vector<int32_t> row_of;  // compact node -> row
    RowsReverse rev;              // the rows' reverse edges (symmetrised search)
    SearchState ss;               // of every search of this thread, rows or whole table
    bool warm = false;
    static SolveScratch& get() {
        thread_local SolveScratch s;
        return s;
    }
    void warmup(int k) {
        if (warm) return;
        warm = true;
        ndc.assign(3 * 16384, 0.0);
        rowc.assign((size_t)16384 * k, 0);
        row_of.assign(16384, -1);
        rev.roff.assign(16385, 0);  // (the symmetrised search's: rare, but its first use is in a timed plan)
        rev.fill.assign(16384, 0);
        rev.radj.assign((size_t)16384 * k, 0);
        ss.begin(16384);
        ss.heap.resize(ss.heap.capacity() / 4);  // (touch part of the heap's storage)
        ss.heap.clear();
    }
};

// EPP_PLAN_TRACE=1 (diagnostics): the fallback's phases on stderr
bool plan_trace() {
    static const bool t = [] {
        const char* e = std::getenv("EPP_PLAN_TRACE");
        return e && std::atoi(e) == 1;
    }();
    return t;
}

// The whole k-NN table of one problem's nodes (device, start and goal first), in phases on
// the area's own stream.  enqueue: k-NN, motion checks straight off the table with the mask
// folded in (failed motions -> -1; the kept edges and those into the goal, node 1, counted).
// counts: the two counts alone (their download queued by enqueue), for a caller that
// searches its rows while the device works.  search: the table down (up to 65535 nodes as u16, 0xFFFF: no edge) with
// the nodes, then A* over the forward edges and, if that does not reach the goal, over the
// symmetrised graph.  Device time, search time and the edge counts go to the problem's out.
class WholeTable {
public:
    struct Counts {
        int64_t kept, into_goal;  // kept edges, kept edges into the goal
    };
    WholeTable(const PlanContext& c, BatchScratch::Area& a, ProblemOut& o) : c_(c), a_(a), o_(o) {}

    void enqueue(const double* d_nodes, int32_t n, const double box[6], bool want_counts = false) {
        t0_ = mark_ = Clock::now();
        const int k = c_.k;
        d_nodes_ = d_nodes;
        n_ = n;
        m_ = (size_t)n * k;
        narrow_ = n <= 65535;
        const size_t ws_bytes = (size_t)epp_knn_workspace_size(n);
        if (BatchScratch::area_dev_bytes(n, k) > a_.dcap || BatchScratch::area_pin_bytes(n, k) > a_.pin.cap)
            throw std::runtime_error("planPath: fallback workspace too small");
        char* dp = static_cast<char*>(a_.dev);
        d_ecnt_ = reinterpret_cast<int64_t*>(dp);
        d_nbr_ = reinterpret_cast<int32_t*>(dp + r256(16));
        d_nbr16_ = narrow_ ? reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(d_nbr_) + r256(m_ * 4)) : nullptr;
        uint8_t* d_ev = reinterpret_cast<uint8_t*>(d_nbr_) + r256(m_ * 4) + r256(m_ * 2);
        d_ws_ = d_ev + r256(m_);
        void* st = a_.stream;
        if (hipMemsetAsync(d_ecnt_, 0, 16, static_cast<hipStream_t>(st)) != hipSuccess)
            throw std::runtime_error("planPath: clearing the edge counts failed");
        check(epp_knn_ws_box(d_nodes, n, k, 0.0, box, box + 3, d_nbr_, d_ws_, ws_bytes, st), "knn");
        const int32_t cp = c_.canPass ? 1 : 0;
        const epp_status ks = check_knn_motions_masked(c_.world, d_nodes, d_nbr_, n, k, cp, d_ev, d_nbr16_, 1, d_ecnt_, st);
        if (ks == EPP_ERR_UNSUPPORTED) {  // (worlds without tile tables: materialised endpoints)
            ThreadScratch& ts = ThreadScratch::get();
            ts.reset(2 * ThreadScratch::rounded(m_ * 24));
            double* d_e1 = static_cast<double*>(ts.carve(m_ * 24));
            double* d_e2 = static_cast<double*>(ts.carve(m_ * 24));
            check(epp_knn_edges(d_nodes, d_nbr_, n, k, d_e1, d_e2, st), "edges");
            check(epp_check_motions(c_.world, d_e1, d_e2, (int64_t)m_, cp, 0, d_ev, st), "motion check");
            check(mask_edges_count_acc(d_nbr_, d_ev, (int64_t)m_, 1, d_ecnt_, st, d_nbr16_), "mask edges");
        } else {
            check(ks, "motion check");
        }
        if (want_counts) check(epp_memcpy_d2h_async(ecnt(), d_ecnt_, 16, st), "download");
        queued_ = Clock::now();
    }

    // Waits for the counts asked of enqueue.  What the caller did since (its own search on
    // the rows, while the device worked) is search time, not device time.
    Counts counts() {
        const auto tr = Clock::now();
        check(epp_stream_sync(a_.stream), "sync");
        const auto tw = Clock::now();
        if (plan_trace())
            std::cerr << "[plan trace] whole table n " << n_ << " for its goal-edge count: " << ms_between(t0_, tw)
                      << " ms (waited " << ms_between(tr, tw) << " ms after the rows' search)"
                      << ", kept edges into the goal " << ecnt()[1] << std::endl;
        o_.ms_search += ms_between(queued_, tr);
        o_.ms_dev += ms_between(mark_, tw) - ms_between(queued_, tr);
        mark_ = tw;
        return take_counts();
    }

    bool search(std::vector<Vec3>& path) {
        const int k = c_.k;
        const int32_t n = n_;
        void* st = a_.stream;
        // the downloads queued back to back, one synchronisation
        char* hp = a_.pin.as<char>();
        double* nodes = reinterpret_cast<double*>(hp + r256(64));
        void* h_tab = hp + r256(64) + r256((size_t)n * 24);
        check(epp_memcpy_d2h_async(ecnt(), d_ecnt_, 16, st), "download");
        check(epp_memcpy_d2h_async(nodes, d_nodes_, (uint64_t)n * 24, st), "download");
        if (narrow_) check(epp_memcpy_d2h_async(h_tab, d_nbr16_, m_ * 2, st), "download");
        else check(epp_memcpy_d2h_async(h_tab, d_nbr_, m_ * 4, st), "download");
        check(epp_stream_sync(st), "sync");
        const bool goal_has_forward_edge = take_counts().into_goal > 0;
        const auto t1 = Clock::now();
        o_.ms_dev += ms_between(mark_, t1);
        Table tab{h_tab, narrow_, k, n};
        const NodePos pos{nodes};
        SearchState& ss = SolveScratch::get().ss;
        // (no forward edge into the goal: the forward pass cannot reach it -- it would only
        // explore start's whole component first; same result, so go straight to the second)
        int r = goal_has_forward_edge ? search_table(ss, tab, pos).r : 0;
        const auto t_fwd = Clock::now();
        if (r != 1) {  // the symmetrised graph: the reverse edges as a CSR, built on the device
            // (counting sort of the masked table; every node's sources ascending, the order of a
            // host build scanning the rows in node order) and downloaded with one synchronisation
            char* rp = reinterpret_cast<char*>(d_ws_) + r256((size_t)epp_knn_workspace_size(n));
            const size_t nb = r256((size_t)(n + 1) * 4);
            int32_t* d_cnt = reinterpret_cast<int32_t*>(rp);
            int32_t* d_fill = reinterpret_cast<int32_t*>(rp + nb);
            int32_t* d_roff = reinterpret_cast<int32_t*>(rp + 2 * nb);
            int32_t* d_radj = reinterpret_cast<int32_t*>(rp + 3 * nb);
            uint16_t* d_radj16 = narrow_ ? reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(d_radj) + r256(m_ * 4)) : nullptr;
            check(reverse_csr(d_nbr_, n, k, d_cnt, d_fill, d_roff, d_radj, d_radj16, st), "reverse edges");
            int32_t* roff = reinterpret_cast<int32_t*>(static_cast<char*>(h_tab) + r256(m_ * 4));
            void* h_radj = reinterpret_cast<char*>(roff) + nb;
            check(epp_memcpy_d2h_async(roff, d_roff, (uint64_t)(n + 1) * 4, st), "download");
            check(epp_stream_sync(st), "sync");
            const int64_t ne = roff[n];
            if (narrow_) check(epp_memcpy_d2h_async(h_radj, d_radj16, (uint64_t)ne * 2, st), "download");
            else check(epp_memcpy_d2h_async(h_radj, d_radj, (uint64_t)ne * 4, st), "download");
            check(epp_stream_sync(st), "sync");
            tab.roff = roff;
            tab.radj = h_radj;
            const auto t_csr = Clock::now();
            const Searched s = search_table(ss, tab, pos);
            r = s.r;
            if (plan_trace())  // (closed: the nodes expanded, so not the goal)
                std::cerr << "[plan trace] whole table n " << n << " forward edge into goal " << goal_has_forward_edge
                          << ": device " << ms_between(t0_, t1) << " ms, forward A* " << ms_between(t1, t_fwd)
                          << " ms, reverse CSR " << ms_between(t_fwd, t_csr) << " ms, symmetrised A* "
                          << ms_between(t_csr, Clock::now()) << " ms (" << s.pops - (r == 1) << " closed), found "
                          << (r == 1) << std::endl;
        }
        path.clear();
        if (r == 1) path = extract_path(ss, pos);
        o_.ms_search += ms_between(t1, Clock::now());
        return r == 1;
    }

private:
    static size_t r256(size_t b) { return BatchScratch::r256(b); }
    int64_t* ecnt() const { return a_.pin.as<int64_t>(); }
    Counts take_counts() {  // (downloaded and synchronised)
        o_.edges_checked = (int64_t)m_;
        o_.edges_valid = ecnt()[0];
        return {ecnt()[0], ecnt()[1]};
    }
    const PlanContext& c_;
    BatchScratch::Area& a_;
    ProblemOut& o_;
    Clock::time_point t0_, queued_, mark_;  // enqueue's start and end; up to where ms_dev is counted
    const double* d_nodes_ = nullptr;       // what enqueue was given, and its parts of the area's device buffer
    int32_t n_ = 0;
    size_t m_ = 0;
    bool narrow_ = false;
    int64_t* d_ecnt_ = nullptr;
    int32_t* d_nbr_ = nullptr;
    uint16_t* d_nbr16_ = nullptr;
    void* d_ws_ = nullptr;
};

// The emitted results of a batch in its pinned block (PlanBatchLayout, epp_internal.h).
struct Emitted {
    const uint64_t* hdr;
    const uint32_t* slots;
    const uint16_t* rows;
    const double* need;
    std::vector<int64_t> first;  // rows are dense in problem order (set once the results are in)
    int S, k;
    const double* d_nodes0;  // the problems' nodes on the device, node_stride apart
    size_t node_stride;
    int64_t hv(int field, int p) const { return (int64_t)hdr[kPbPerSeg + field * S + p]; }
    const double* d_nodes(int p) const { return d_nodes0 + (size_t)p * node_stride * 3; }
};

// The symmetrised search on the rows.  The reference's next step after a failed forward
// search is the symmetrised graph (WholeTable::search); search_rows says why the rows' own
// reverse edges suffice while the pops stay within the bound.  Valid only once the whole
// table's forward search is known to fail (solve_problem, census).
int rows_symmetrised(SolveScratch& sc, const Rows& g, double bound, ProblemOut& o) {
    sc.rev.build(g);
    const Searched s = search_rows(sc.ss, g, NodePos{sc.ndc.data()}, bound, &sc.rev);
    o.pops += s.pops;
    o.why = s.r == -1 ? 5 : s.r == 0 ? 6 : -1;
    o.symmetrised = s.r == 1 ? 1 : 0;
    return s.r;
}

// No kept edge into the goal among the rows: the whole table's forward search fails if no
// node outside the rows keeps one either.  Its masked k-NN (on the device) counts them
// while the symmetrised search runs on the rows here; with none, that search decides and
// the table is not downloaded.  wt: enqueued, its counts asked for.
void census(int p, double bound, const Rows& g, WholeTable& wt, ProblemOut& o) {
    SolveScratch& sc = SolveScratch::get();
    o.fallback = 1;
    o.why = 2;
    const auto ts0 = Clock::now();
    const int r2 = rows_symmetrised(sc, g, bound, o);  // (o.why: 5 / 6 when it fails)
    if (plan_trace())
        std::cerr << "[plan trace] problem " << p << ": symmetrised search on " << o.restricted_rows << " rows / "
                  << g.m << " nodes: " << o.pops << " closed, " << ms_between(ts0, Clock::now()) << " ms, result " << r2
                  << " (copies before: " << o.ms_restricted << " ms)" << std::endl;
    const WholeTable::Counts cnt = wt.counts();
    // why the whole table was searched: a kept goal edge outside the rows (2), else the
    // rows' symmetrised search failed (5 / 6, set by it)
    if (cnt.into_goal > 0) o.why = 2;
    if (cnt.into_goal == 0 && r2 == 1) {
        o.path = extract_path(sc.ss, NodePos{sc.ndc.data()});
        o.found = true;
        o.fallback = 0;
        o.census = 1;
        o.rows_down = o.restricted_rows;
    } else {
        o.found = wt.search(o.path);
        o.rows_down = o.n;
        o.symmetrised = 0;
    }
}

// One problem: the restricted search on its emitted rows, else the whole table.
// kbox: the whole table's k-NN box.
void solve_problem(const Emitted& em, int p, const PlanSeg& seg, const double* kbox, WholeTable& wt, ProblemOut& o) {
    const int k = em.k;
    const int64_t n = em.hv(3, p);
    o.n = n;
    const int64_t packed = em.hv(0, p);
    const int64_t m = std::min<int64_t>(em.hv(4, p), seg.need_cap);
    const auto t0 = Clock::now();
    int r = 0;
    // (restricted: rows within capacity, exact (hv 5), node ids in u16; start and goal are
    // compact indices 0 and 1: rows of their own)
    if (seg.cap > 0) o.why = (n > 65535 || packed > seg.cap || m < 2) ? 0 : em.hv(5, p) != 0 ? 1 : -1;
    if (seg.cap > 0 && n <= 65535 && packed <= seg.cap && em.hv(5, p) == 0 && m >= 2) {
        // this problem's rows and referenced nodes (compact indices: node order), copied
        // out of the pinned buffer first: the device wrote them, so they are in no CPU
        // cache, and A*'s scattered reads would each wait out a DRAM access (~70 ns; the
        // slowest search of a call took 0.15 ms for ~130 pops), where one sequential copy
        // streams them in
        const int64_t first = em.first[p], nrow = em.first[p + 1] - first;
        SolveScratch& sc = SolveScratch::get();
        grow_to(sc.ndc, (size_t)m * 3, 3 * 16384);
        grow_to(sc.rowc, (size_t)nrow * k, (size_t)16384 * k);
        std::memcpy(sc.ndc.data(), em.need + 3 * seg.need_off, (size_t)m * 24);
        std::memcpy(sc.rowc.data(), em.rows + (size_t)first * k, (size_t)nrow * k * 2);
        o.ms_copy = ms_between(t0, Clock::now());
        grow_to(sc.row_of, (size_t)m, 16384);
        std::fill(sc.row_of.begin(), sc.row_of.begin() + m, -1);
        for (int64_t sl = 0; sl < nrow; ++sl) sc.row_of[em.slots[first + sl] & 0xFFFFu] = (int32_t)sl;
        const Rows g{sc.rowc.data(), sc.row_of.data(), k, m};
        const NodePos pos{sc.ndc.data()};
        // (no kept edge into the goal among the rows: the forward search on them cannot
        // reach it -- the goal-edge count below decides instead, r = -1)
        const bool goal_edges = em.hv(2, p) > 0;
        const Searched fwd = goal_edges ? search_rows(sc.ss, g, pos, seg.bound) : Searched{-1, 0};
        r = fwd.r;
        o.restricted_rows = packed;
        o.pops = fwd.pops;
        o.nodes = m;
        o.why = r == -1 ? 3 : r == 0 ? 4 : -1;
        if (r == 0) {
            // The forward search exhausted its component with every pop inside the bound:
            // every node it reached has its row here, so the whole table's forward search
            // reaches the same nodes and fails too.
            r = rows_symmetrised(sc, g, seg.bound, o);
        } else if (!goal_edges) {
            o.ms_restricted = ms_between(t0, Clock::now());
            o.ms_search += o.ms_restricted;
            wt.enqueue(em.d_nodes(p), (int32_t)n, kbox, /*want_counts=*/true);
            census(p, seg.bound, g, wt, o);
            return;
        }
        if (r == 1) {
            o.path = extract_path(sc.ss, pos);
            o.found = true;
            o.edges_checked = packed * k;
            o.edges_valid = em.hv(1, p);
            o.rows_down = packed;
        }
    }
    o.ms_restricted = ms_between(t0, Clock::now());
    o.ms_search += o.ms_restricted;
    if (r != 1) {
        o.fallback = seg.cap > 0 ? 1 : 0;
        wt.enqueue(em.d_nodes(p), (int32_t)n, kbox);
        o.found = wt.search(o.path);
        o.rows_down += n;
    }
}

// The solvers of one batch: W - 1 pool threads and the caller as worker 0.  The threads are
// started (here) before the launch and wait for the results, so their wake-up overlaps the
// device stages; then the W solvers pull problems in order.  go: 1 results in, -1 no
// results (the launch failed: the destructor releases the threads without solving).  A
// thread spins for at most kSpinUs (a warm batch is ~0.17 ms: the spin keeps the wake-up
// off the critical path) and then blocks on go_cv, so a slow batch (the cold first plan's
// warm-up, a hung device) does not keep W - 1 cores busy.
template <class Solve>  // solve(p, w): problem p on worker w's area
class SolveCrew {
public:
    SolveCrew(size_t W, int S, int k, Solve& solve) : S_(S), k_(k), solve_(solve), err_(S), pending_(W - 1) {
        int devno = 0;
        if (hipGetDevice(&devno) != hipSuccess) devno = 0;
        for (size_t t = 1; t < W; ++t) plan_pool().submit([this, devno, t] { wait_then_drain(devno, t); });
    }
    ~SolveCrew() {
        if (go_.load(std::memory_order_acquire) == 0) set_go(-1);
        join();  // (no thread outlives what solve refers to)
    }
    // The results are in: solves every problem (the caller drains as worker 0), joins the
    // threads and rethrows the first problem's stored exception.
    void run() {
        set_go(1);
        drain(0);
        join();
        for (const auto& e : err_)
            if (e) std::rethrow_exception(e);
    }

private:
    void set_go(int v) {
        {
            std::lock_guard<std::mutex> lk(go_mu_);
            go_.store(v, std::memory_order_release);
        }
        go_cv_.notify_all();
    }
    void drain(size_t w) {
        SolveScratch::get().warmup(k_);
        for (int p = next_++; p < S_; p = next_++) {
            try {
                solve_(p, w);
            } catch (...) {
                err_[p] = std::current_exception();
            }
        }
    }
    void wait_then_drain(int devno, size_t t) {
        (void)hipSetDevice(devno);
        constexpr int64_t kSpinUs = 400;
        const auto ts = Clock::now();
        int g;
        for (uint32_t i = 0; (g = go_.load(std::memory_order_acquire)) == 0; ++i) {
            _mm_pause();
            if ((i & 255) == 255 && Clock::now() - ts > std::chrono::microseconds(kSpinUs)) {
                std::unique_lock<std::mutex> lk(go_mu_);
                go_cv_.wait(lk, [&] { return go_.load(std::memory_order_acquire) != 0; });
            }
        }
        if (g > 0) drain(t);
        std::lock_guard<std::mutex> lk(done_mu_);
        if (--pending_ == 0) done_cv_.notify_all();
    }
    void join() {
        std::unique_lock<std::mutex> lk(done_mu_);
        done_cv_.wait(lk, [&] { return pending_ == 0; });
    }
    const int S_, k_;
    Solve& solve_;
    std::vector<std::exception_ptr> err_;
    std::atomic<int> go_{0}, next_{0};
    std::mutex go_mu_, done_mu_;
    std::condition_variable go_cv_, done_cv_;
    size_t pending_;
};

// Queues the batch's device stages and waits for the emitted results; returns the time
// since t0 at which every stage was queued.
double launch_and_wait(const PlanContext& c, const PlanBatchLayout& L, BatchScratch& bs, Clock::time_point t0) {
    char* H = bs.host();
    void* st = bs.stream();
    const uint32_t seq = bs.next_seq();
    check(plan_batch_launch(c.world, c.canPass ? 1 : 0, c.box.lo, c.box.hi, L, bs.dev(), H, seq, st), "planner batch");
    const double ms_enqueue = ms_between(t0, Clock::now());
    // the emit's completion slots (polled: no stream synchronisation), the stream's
    // state every ~1k polls (a failed launch ends the wait)
    static const bool sync_wait = [] {  // (A/B knob: EPP_PB_SYNC=1 synchronises the stream instead)
        const char* e = std::getenv("EPP_PB_SYNC");
        return e && std::atoi(e) == 1;
    }();
    if (sync_wait) check(epp_stream_sync(st), "sync");
    // (a deadline: a batch that has not completed in kBatchDeadlineS raises instead of
    // polling forever.  Hazard: its kernels may still be running, and this thread's
    // BatchScratch is reused by the next call; if that call grows the scratch, it frees
    // buffers that the still-running kernels may write)
    constexpr double kBatchDeadlineS = 30.0;
    const WaitResult r = wait_done(reinterpret_cast<const uint32_t*>(H + L.h_done), L.done_n, seq,
                                   static_cast<hipStream_t>(st), kBatchDeadlineS);
    if (r.kind == WaitResult::kDeadline)
        throw std::runtime_error("planner batch: not complete after 30 s (device hung?)");
    if (r.kind == WaitResult::kHipError)
        throw std::runtime_error(std::string("planner batch: ") + hipGetErrorString(r.err));
    if (r.kind == WaitResult::kNoSlots)
        throw std::runtime_error("planner batch: completed without its completion slots");
    plan_batch_trace_print();
    return ms_enqueue;
}
}  // namespace

BatchSolution solve_batch(const PlanContext& c, std::vector<PlanSeg>& segs, const std::vector<std::array<double, 6>>& kbox,
                          Clock::time_point t0) {
    const int S = (int)segs.size(), k = c.k;
    const int64_t nmax = c.box.nmax;
    // ---- layout and scratch --------------------------------------------------------------
    const PlanBatchLayout L = plan_batch_layout(S, nmax - 2, k, segs.data());
    BatchScratch& bs = BatchScratch::get();
    bs.ensure(L.dev_bytes, L.host_bytes);
    // W concurrent solvers (the caller + W - 1 pool threads), each with its fallback buffers
    const size_t W = std::min((size_t)S, (size_t)std::max(1, c.threads));  // (threads: 16 by default)
    bs.ensure_areas(W, nmax, k);
    char* H = bs.host();
    std::memcpy(H + L.h_seg, segs.data(), sizeof(PlanSeg) * S);
    Emitted em{reinterpret_cast<const uint64_t*>(H + L.h_hdr), reinterpret_cast<const uint32_t*>(H + L.h_slot),
               reinterpret_cast<const uint16_t*>(H + L.h_rows), reinterpret_cast<const double*>(H + L.h_need),
               std::vector<int64_t>(S + 1, 0), S, k,
               reinterpret_cast<const double*>(static_cast<const char*>(bs.dev()) + L.o_nodes), (size_t)L.NS};
    BatchSolution sol;
    sol.out.resize(S);
    auto solve = [&](int p, size_t w) {
        WholeTable wt(c, bs.area(w), sol.out[p]);
        solve_problem(em, p, segs[p], kbox[p].data(), wt, sol.out[p]);
    };
    SolveCrew<decltype(solve)> crew(W, S, k, solve);
    // ---- launch and wait -----------------------------------------------------------------
    sol.ms_enqueue = launch_and_wait(c, L, bs, t0);
    for (int p = 0; p < S; ++p) em.first[p + 1] = em.first[p] + std::min<int64_t>(em.hv(0, p), segs[p].cap);
    // Cold areas (this thread's first plans): one whole-table search on problem 0's
    // nodes, so that the fallback's first launches and transfers are paid here, in the
    // cold first plan, rather than by the first search that falls back.
    for (size_t a = 0; a < W; ++a) {
        BatchScratch::Area& ar = bs.area(a);
        if (!ar.cold) continue;
        ar.cold = false;
        ProblemOut unused;
        WholeTable wt(c, ar, unused);
        wt.enqueue(em.d_nodes(0), (int32_t)em.hv(3, 0), kbox[0].data());
        (void)wt.search(unused.path);
    }
    sol.ms_batch = ms_between(t0, Clock::now());
    // ---- solve ---------------------------------------------------------------------------
    crew.run();
    return sol;
}

}  // namespace epp
