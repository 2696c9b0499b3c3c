// host_dbg_planner.cpp — debug entries (not part of include/epp.h; declared in eppamd/capi.py)
// that hand the tests what the planner's device stages produce, below the level of a
// finished path:
//
//   epp_dbg_plan_batch  : one batch through plan_batch_layout / plan_batch_launch as the
//                         product drives them, the emitted pinned block and each problem's
//                         node list copied out.  No PathPlanner, no solver threads, no
//                         fallback: what the stages wrote is what the caller sees.
//   epp_dbg_reverse_csr : epp::reverse_csr of a device table, roff / radj / radj16 copied out.
//   epp_dbg_knn_motions_masked / _rows : epp::check_knn_motions_masked / _rows on the caller's
//                         device buffers, nothing allocated or cleared: what k_motions_v5's
//                         MotionMask tail writes, and leaves alone, is what the caller reads.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "epp_internal.h"
#include "launch_helpers.h"

using namespace epp;

namespace {
struct DevBlock {  // hipMalloc (256-byte aligned), freed on scope exit
    void* p = nullptr;
    ~DevBlock() {
        if (p) (void)hipFree(p);
    }
    bool alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 256)) == hipSuccess; }
};
struct PinBlock {  // hipHostMalloc (page aligned)
    void* p = nullptr;
    ~PinBlock() {
        if (p) (void)hipHostFree(p);
    }
    bool alloc(size_t bytes) { return hipHostMalloc(&p, std::max<size_t>(bytes, 256), hipHostMallocDefault) == hipSuccess; }
};
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};
epp_status fail(epp_status st, const char* msg) {
    set_error(msg);
    return st;
}
epp_status hip_fail(const char* what) {  // a HIP call failed: its error as a status
    const epp_status st = launch_error(what);
    return st != EPP_OK ? st : fail(EPP_ERR_HIP, what);
}
}  // namespace

// One batch of S problems (ns samples each) through the batched planner's device stages.
// Per problem p the caller-filled fields of PlanSeg: seeds[p], ends[6 p] (s, g), bounds[2 p]
// (bound, gbound), gbox[6 p] (glo, ghi), h[p], cap[p].  The batch runs n_runs times on one
// workspace, run r with seqs[r]; fill bit 0: the device and the pinned block hold 0xFF bytes
// before the first run (else zeros); bit 1: the pinned block's emitted part (everything but the
// problems) is overwritten with 0xFF between runs.  The outputs are the last run's, copied
// after the stream is synchronised:
//   hdr (3 + 6 S u64), slots (u32, slots_cap >= rows capacity rounded up to 4), rows (u16,
//   slots_cap x k), need (3 need_slots doubles, need_slots >= every problem's need_off +
//   need_cap), row_off / need_off (i64 per problem), need_cap (i32 per problem), done (u32,
//   done_cap >= the completion slots), nodes (S x (ns + 2) x 3 doubles: problem p's first
//   hdr[3 + 3 S + p] nodes from the device), meta: cap_total, need slots, completion slots,
//   ns_log, device bytes, pinned bytes.
// EPP_ERR_UNSUPPORTED: some cap > 0 on a world the rows' motion check cannot run on;
// EPP_ERR_CAPACITY: an output buffer too small for the layout (meta is filled).
extern "C" epp_status epp_dbg_plan_batch(const epp_world* world, int32_t can_pass_gate, const double lo[3],
                                         const double hi[3], int64_t ns, int32_t k, int32_t S, const uint64_t* seeds,
                                         const double* ends, const double* bounds, const double* gbox,
                                         const double* h, const int32_t* cap, const uint32_t* seqs, int32_t n_runs,
                                         int32_t fill, uint64_t* hdr, uint32_t* slots, uint16_t* rows,
                                         int64_t slots_cap, double* need, int64_t need_slots, int64_t* row_off,
                                         int64_t* need_off, int32_t* need_cap, uint32_t* done, int32_t done_cap,
                                         double* nodes, int64_t meta[6]) {
    if (!world || !lo || !hi || ns < 1 || S < 1 || S > 64 || (k != 4 && k != 8 && k != 16) || !seeds || !ends ||
        !bounds || !gbox || !h || !cap || !seqs || n_runs < 1 || !hdr || !slots || !rows || !need || !row_off ||
        !need_off || !need_cap || !done || !nodes || !meta || slots_cap < 0 || need_slots < 0)
        return fail(EPP_ERR_INVALID_ARGUMENT, "epp_dbg_plan_batch: invalid argument");
    std::vector<PlanSeg> segs((size_t)S);
    bool restricted = false;
    for (int p = 0; p < S; ++p) {
        PlanSeg& q = segs[(size_t)p];
        q = PlanSeg{};
        q.seed = seeds[p];
        for (int d = 0; d < 3; ++d) {
            q.s[d] = ends[6 * p + d];
            q.g[d] = ends[6 * p + 3 + d];
            q.glo[d] = gbox[6 * p + d];
            q.ghi[d] = gbox[6 * p + 3 + d];
        }
        q.bound = bounds[2 * p];
        q.gbound = bounds[2 * p + 1];
        q.h = h[p];
        q.cap = cap[p];
        restricted = restricted || cap[p] > 0;
    }
    if (restricted && !knn_motions_rows_supported(world))
        return fail(EPP_ERR_UNSUPPORTED, "epp_dbg_plan_batch: the world has no tile tables for the rows' motion check");
    const PlanBatchLayout L = plan_batch_layout(S, ns, k, segs.data());
    const int64_t capr = ((int64_t)L.cap_total + 3) & ~int64_t(3);
    meta[0] = L.cap_total;
    meta[1] = L.need_cap;
    meta[2] = L.done_n;
    meta[3] = L.ns_log;
    meta[4] = (int64_t)L.dev_bytes;
    meta[5] = (int64_t)L.host_bytes;
    if (slots_cap < capr || need_slots < L.need_cap || done_cap < L.done_n)
        return fail(EPP_ERR_CAPACITY, "epp_dbg_plan_batch: an output buffer is smaller than the layout");
    DevBlock dev;
    PinBlock host;
    Stream st;
    if (!dev.alloc(L.dev_bytes) || !host.alloc(L.host_bytes) || hipStreamCreate(&st.s) != hipSuccess)
        return hip_fail("epp_dbg_plan_batch: allocation");
    char* H = static_cast<char*>(host.p);
    // (the workspace holds known bytes either way: what a stage leaves unwritten is the same in every run)
    if (hipMemsetAsync(dev.p, (fill & 1) ? 0xFF : 0, L.dev_bytes, st.s) != hipSuccess ||
        hipStreamSynchronize(st.s) != hipSuccess)
        return hip_fail("epp_dbg_plan_batch: fill");
    std::memset(H, (fill & 1) ? 0xFF : 0, L.host_bytes);
    std::memcpy(H + L.h_seg, segs.data(), sizeof(PlanSeg) * (size_t)S);
    for (int r = 0; r < n_runs; ++r) {
        if (r > 0 && (fill & 2)) std::memset(H + L.h_hdr, 0xFF, L.host_bytes - L.h_hdr);
        if (const epp_status e = plan_batch_launch(world, can_pass_gate, lo, hi, L, dev.p, H, seqs[r], st.s)) return e;
        if (hipStreamSynchronize(st.s) != hipSuccess) return hip_fail("epp_dbg_plan_batch: synchronise");
    }
    std::memcpy(hdr, H + L.h_hdr, (size_t)L.nctr * 8);
    std::memcpy(slots, H + L.h_slot, (size_t)capr * 4);
    std::memcpy(rows, H + L.h_rows, (size_t)capr * k * 2);
    std::memcpy(need, H + L.h_need, (size_t)L.need_cap * 24);
    std::memcpy(done, H + L.h_done, (size_t)L.done_n * 4);
    for (int p = 0; p < S; ++p) {
        row_off[p] = segs[(size_t)p].row_off;
        need_off[p] = segs[(size_t)p].need_off;
        need_cap[p] = segs[(size_t)p].need_cap;
        const int64_t n = std::min<int64_t>((int64_t)hdr[kPbPerSeg + 3 * S + p], ns + 2);
        if (n > 0 &&
            hipMemcpy(nodes + (size_t)p * (size_t)(ns + 2) * 3,
                      static_cast<const char*>(dev.p) + L.o_nodes + (size_t)p * (size_t)L.NS * 24, (size_t)n * 24,
                      hipMemcpyDeviceToHost) != hipSuccess)
            return hip_fail("epp_dbg_plan_batch: nodes");
    }
    return EPP_OK;
}

// epp::reverse_csr of the device table nbr (n x k, int32, -1: none; every other entry in
// [0, n), checked here): roff (n + 1), radj (the first roff[n] of its n k slots) and, for
// n <= 65535 and radj16 != NULL, radj16 copied into the caller's host arrays.
extern "C" epp_status epp_dbg_reverse_csr(const int32_t* nbr, int32_t n, int32_t k, int32_t* roff, int32_t* radj,
                                          uint16_t* radj16) {
    if (!nbr || n < 1 || k < 1 || !roff || !radj)
        return fail(EPP_ERR_INVALID_ARGUMENT, "epp_dbg_reverse_csr: invalid argument");
    const size_t m = (size_t)n * (size_t)k;
    {
        std::vector<int32_t> tab(m);
        if (hipMemcpy(tab.data(), nbr, m * 4, hipMemcpyDeviceToHost) != hipSuccess) return hip_fail("epp_dbg_reverse_csr");
        for (const int32_t v : tab)
            if (v < -1 || v >= n) return fail(EPP_ERR_INVALID_ARGUMENT, "epp_dbg_reverse_csr: entry out of range");
    }
    const bool narrow = radj16 != nullptr && n <= 65535;
    DevBlock cnt, fil, off, adj, adj16;
    Stream st;
    if (!cnt.alloc((size_t)n * 4) || !fil.alloc((size_t)n * 4) || !off.alloc((size_t)(n + 1) * 4) || !adj.alloc(m * 4) ||
        (narrow && !adj16.alloc(m * 2)) || hipStreamCreate(&st.s) != hipSuccess)
        return hip_fail("epp_dbg_reverse_csr: allocation");
    if (const epp_status e = reverse_csr(nbr, n, k, static_cast<int32_t*>(cnt.p), static_cast<int32_t*>(fil.p),
                                         static_cast<int32_t*>(off.p), static_cast<int32_t*>(adj.p),
                                         narrow ? static_cast<uint16_t*>(adj16.p) : nullptr, st.s))
        return e;
    if (hipStreamSynchronize(st.s) != hipSuccess) return hip_fail("epp_dbg_reverse_csr: synchronise");
    if (hipMemcpy(roff, off.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return hip_fail("epp_dbg_reverse_csr");
    const int64_t ne = std::min<int64_t>(std::max<int32_t>(roff[n], 0), (int64_t)m);
    if (ne > 0 && hipMemcpy(radj, adj.p, (size_t)ne * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return hip_fail("epp_dbg_reverse_csr");
    if (narrow && ne > 0 && hipMemcpy(radj16, adj16.p, (size_t)ne * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return hip_fail("epp_dbg_reverse_csr");
    return EPP_OK;
}

// epp::check_knn_motions_masked on the caller's device buffers (nbr is rewritten in place);
// the callee's status, unchanged.
extern "C" epp_status epp_dbg_knn_motions_masked(const epp_world* world, const double* nodes, int32_t* nbr, int32_t n,
                                                 int32_t k, int32_t can_pass_gate, uint8_t* valid, uint16_t* out16,
                                                 int32_t target, int64_t* count, void* stream) {
    return check_knn_motions_masked(world, nodes, nbr, n, k, can_pass_gate, valid, out16, target, count, stream);
}

extern "C" int32_t epp_dbg_knn_motions_rows_supported(const epp_world* world) {
    return knn_motions_rows_supported(world) ? 1 : 0;
}

// epp::check_knn_motions_rows on the caller's device buffers, the marks built as
// plan_batch_launch builds them (mark / pkept / pgoal / ns_log / nprob); mark == NULL: no
// marks (the packed rows of one problem), pkept / pgoal / ns_log / nprob are then unused.
// The callee's status, unchanged.
extern "C" epp_status epp_dbg_knn_motions_rows(const epp_world* world, const double* nodes, int32_t* rows32,
                                               const int32_t* ids32, const int64_t* rows_n, int32_t cap, int32_t k,
                                               int32_t can_pass_gate, uint8_t* valid, uint16_t* out16, int32_t target,
                                               int64_t* count, uint8_t* mark, uint64_t* pkept, uint64_t* pgoal,
                                               int32_t ns_log, int32_t nprob, void* stream) {
    MotionMask marks;
    marks.mark = mark;
    marks.pkept = reinterpret_cast<unsigned long long*>(pkept);
    marks.pgoal = reinterpret_cast<unsigned long long*>(pgoal);
    marks.ns_log = ns_log;
    marks.nprob = nprob;
    return check_knn_motions_rows(world, nodes, rows32, ids32, rows_n, cap, k, can_pass_gate, valid, out16, target,
                                  count, stream, mark ? &marks : nullptr);
}
