// minsnap_refit.hip — the single-track fused refit (the 50 Hz latency path) for gfx950.
//
// poly_traj::generateTrajectory for one track in ONE launch, reading its inputs from and
// writing the rows to pinned host memory (no copies).  The host has already run the two
// sequential parts, which a GPU lane runs slowly (~65 ns per dependent step): the segment
// times (Nfabian with the host's libm, as the reference) and Trajectory::evaluateRange's
// `acc += dt` recurrence (sample times and segments, exact).  G workgroups each own a
// slice of the rows; every one of them solves the (small) min-snap problem itself with
// those times (solve_track, minsnap_solve.h — the same arithmetic in every one of them, so
// the same coefficients in all G; NOT the batch kernel's bits: k_minsnap (minsnap.hip) runs
// solve_track with 64 threads and the refinement step, this path with 256 and without it, so
// the two fits differ in the last bits, each within the fit's accuracy —
// tests/test_gpu_sample_batch.py) while its slice's sample data arrives from the host, then
// evaluates its rows (Polynomial::evaluate) and writes them to the host: G CUs writing in
// parallel (one CU's PCIe writes are slow) and no hand-off of the coefficients between
// workgroups.  Completion is published in host memory (workgroup 0: the status; every
// workgroup: its slot) and polled by the host instead of synchronising the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "minsnap_kernels.h"
#include "minsnap_solve.h"
#include "small_body.h"
#include "stream_bufs.h"

namespace epp {
namespace {

constexpr int kRefitArgW = 41;  // tracks up to this many waypoints pass wp, v0, a0, T as kernel arguments
constexpr int kRefitMaxWriters = 16;
struct RefitArgs {
    const double* in;  // host-mapped: [wp (W x 3) | v0 (3) | a0 (3) | T (M)] | t_in (R) | t (R) | segment (R, int32)
    int32_t W;
    int32_t R;         // rows
    int32_t writers;   // G (>= 1)
    uint32_t seq;      // this call's number (completion words hold it)
    double t0;         // startTimeOffset
    double* out;       // host-mapped: R x 10 rows
    int64_t* info;     // host-mapped: [status]
    uint32_t* done;    // host-mapped: the workgroups' completion slots
    double* scratch;   // device: G x segment scratch (tracks longer than kMaxLdsSeg)
    int32_t big;       // (!LDS) the vertex values, right-hand sides, times and coefficients
                       // in the global scratch too (tracks whose LDS part would not fit)
    int32_t refine;    // one step of iterative refinement in the solve (solve_track)
    double small[3 * kRefitArgW + 6 + kRefitArgW - 1];  // wp | v0 | a0 | T when W <= kRefitArgW
};
constexpr int kRefitBlock = 256;
constexpr int kRefitRowChunk = 128;  // rows per round (LDS staged)
__host__ __device__ inline size_t refit_in_doubles(int W, int R) {  // (+ 3: row 0 readable when R = 0)
    return (size_t)3 * W + 6 + (W - 1) + 2 * (size_t)R + ((size_t)R + 1) / 2 + 3;
}
__host__ __device__ inline size_t refit_nin_even(int W) { return ((size_t)3 * W + 6 + (W - 1) + 1) & ~size_t(1); }
// LDS doubles: flag (2) | constants | wp, v0, a0, T | solve scratch | coefficients |
// sample chunk (t_in, t, segment) | row chunk.  big: the vertex values, right-hand sides,
// times and coefficients live in the global scratch; LDS keeps the lane exchange (kXch).
// (A refit workgroup's dynamic LDS stays within kLdsBudget, 150 KB, of the 160 KB a CU has.)
__host__ __device__ inline size_t refit_lds_doubles(int M, bool lds, bool big = false) {
    return 2 + kNC + refit_nin_even(M + 1) + (lds ? (size_t)M * Seg::kSize : 0) +
           (big ? (size_t)kXch : vertex_doubles(M) + (size_t)M * 30) + (size_t)kRefitRowChunk * 3 + 2 +
           (size_t)kRefitRowChunk * 10;
}
// global scratch doubles per writer: the segment scratch, and (big) the vertex values,
// right-hand sides, times and coefficients
__host__ __device__ inline size_t refit_scr_doubles(int M, bool big) {
    return (size_t)M * Seg::kSize + (big ? vertex_doubles(M) - kXch + (size_t)M * 30 : 0);
}

template <bool LDS>
__device__ __forceinline__ void refit_body(const RefitArgs& a, int g, double* smem) {
    const int tid = threadIdx.x, W = a.W, M = W - 1, R = a.R;
    const double* h_tin = a.in + 3 * W + 6 + M;
    const double* h_tac = h_tin + R;
    const int32_t* h_seg = reinterpret_cast<const int32_t*>(h_tac + R);
    int* s_err = reinterpret_cast<int*>(smem);
    double* kc = smem + 2;
    double* P = kc + kNC;  // wp | v0 | a0 | T
    double* const after_p = P + refit_nin_even(W);  // (LDS)
    const bool big = !LDS && a.big;
    double* scr = after_p;
    double* dv = LDS ? scr + (size_t)M * Seg::kSize : scr;
    if (!LDS) {
        scr = a.scratch + (size_t)g * refit_scr_doubles(M, big);
        if (big) dv = scr + (size_t)M * Seg::kSize;
    }
    double* rhs = dv + (size_t)(M + 1) * 15;
    double* Tm = rhs + (size_t)(M + 1) * 12;
    double* xch = big ? after_p : Tm + M;  // the solve's lane exchange: always LDS
    double* C = big ? Tm + M : xch + kXch;  // coefficients (M x 3 x 10)
    double* s_tin = big ? xch + kXch : C + (size_t)M * 30;
    double* s_tac = s_tin + kRefitRowChunk;
    int32_t* s_seg = reinterpret_cast<int32_t*>(s_tac + kRefitRowChunk);
    double* rbuf = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(s_tac + 2 * kRefitRowChunk) + 15) &
                                             ~uintptr_t(15));
    const int per = (R + a.writers - 1) / a.writers;
    const int r0 = min(R, g * per), r1 = min(R, r0 + per);
    EPP_TL(0);
    // every input load in flight at once: the constants, the problem (kernel arguments or
    // host memory) and this slice's first sample chunk (host memory)
    // (unconditional loads at clamped addresses: no branches, so the stores below wait
    // with counted vmcnt for their own loads only and the host reads stay in flight)
    const int nin = 3 * W + 6 + M;
    const double* src = W <= kRefitArgW ? a.small : a.in;
    const double cv = cC[min(tid, kNC - 1)];
    double pv[(3 * kRefitArgW + 6 + kRefitArgW - 1 + kRefitBlock - 1) / kRefitBlock];
    constexpr int kPv = sizeof(pv) / sizeof(double);
#pragma unroll
    for (int q = 0; q < kPv; ++q) pv[q] = src[min(tid + q * kRefitBlock, nin - 1)];
    auto fetch = [&](int c0, int cnt) {  // sample data of rows [c0, c0 + cnt) (host reads)
        if (tid < cnt) {
            s_tin[tid] = h_tin[c0 + tid];
            s_tac[tid] = h_tac[c0 + tid];
            s_seg[tid] = h_seg[c0 + tid];
        }
    };
    // the first chunk's sample data is loaded now and kept in registers until the solve
    // is done (the host pads the input so row 0 is readable even when R = 0)
    const int cnt0 = min(kRefitRowChunk, r1 - r0);
    const int fr = r0 + min(tid, max(cnt0 - 1, 0));
    const double f_tin = h_tin[fr], f_tac = h_tac[fr];
    const int32_t f_seg = h_seg[fr];
    if (tid < kNC) kc[tid] = cv;
#pragma unroll
    for (int q = 0; q < kPv; ++q)
        if (tid + q * kRefitBlock < nin) P[tid + q * kRefitBlock] = pv[q];
    for (int e = kPv * kRefitBlock + tid; e < nin; e += kRefitBlock) P[e] = src[e];  // (long tracks)
    if (tid == 0) *s_err = 0;
    block_sync<LDS>();
    EPP_TL(8);
    const int st = solve_track<kRefitBlock, LDS>(kc, P, M, 0.0, 0.0, P + 3 * W, P + 3 * W + 3, P + 3 * W + 6, scr, dv,
                                            rhs, Tm, xch, s_err, nullptr, C, a.refine != 0);
    EPP_TL(7);
    if (tid < cnt0) {
        s_tin[tid] = f_tin;
        s_tac[tid] = f_tac;
        s_seg[tid] = f_seg;
    }
    __syncthreads();  // coefficients complete
    if (st == 0) {
        for (int c0 = r0; c0 < r1; c0 += kRefitRowChunk) {
            const int cnt = min(kRefitRowChunk, r1 - c0);
            if (c0 != r0) {
                __syncthreads();  // the previous chunk copied out
                fetch(c0, cnt);
                __syncthreads();
            }
            if (tid < cnt) {
                const double* cs = C + (size_t)s_seg[tid] * 30;
                const double tin = s_tin[tid];
                double* r = rbuf + (size_t)tid * 10;
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int q = 0; q < 3; ++q) r[3 * d + q] = poly_eval(kc + kCB, cs + d * N, tin, q);
                r[9] = s_tac[tid] + a.t0;  // sampling_times[i] + startTimeOffset
            }
            __syncthreads();
            // contiguous 16-byte stores: a wave writes 1 KB runs
            const double2* src2 = reinterpret_cast<const double2*>(rbuf);
            double2* dst2 = reinterpret_cast<double2*>(a.out + (size_t)c0 * 10);
            for (int q = tid; q < cnt * 5; q += kRefitBlock) dst2[q] = src2[q];
        }
    }
    EPP_TL(13);
    // completion: this slice's rows and workgroup 0's status (stored by the lane that
    // publishes: slot 0 holding seq implies the status) are visible system-wide before the
    // slot is
    if (tid == 0 && g == 0) a.info[0] = st;
    publish_done(a.done + g, a.seq);
}

template <bool LDS>
__global__ __launch_bounds__(kRefitBlock) void k_refit(RefitArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    refit_body<LDS>(a, blockIdx.x, smem);
}

// ---- the C5 online step in one launch: A11 check + refit --------------------------------
// PathPlanner::checkTrajectoryValidity of the lookahead rows against the world
// (World::checkPointValidity(p, minDistance), src/World.cpp:106-128, src/PathPlanner.cpp:
// 267-280) and the refit of the moved waypoints (poly_traj::generateTrajectory) are
// independent: workgroups [0, writers) run the refit (refit_body), workgroups [writers,
// writers + check groups) the brute-force minDistance check of k_states_small
// (states_small_body, small_body.h) over the pinned points, flags into pinned memory.  Every
// workgroup publishes `seq` in its completion slot: one launch, one host poll for both.
static_assert(kRefitBlock == kSmallBlock, "one block size for both parts");
struct CheckArgs {
    const double* recs;  // OBB records (device blob or pinned host copy: SmallWorld)
    int32_t n_obb, per;
    double rg, ro, md;
    const double* xyz;   // host-mapped: n x 3
    int64_t n;
    uint8_t* valid;      // host-mapped: n flags
};

template <bool LDS>
__global__ __launch_bounds__(kRefitBlock) void k_check_refit(RefitArgs a, CheckArgs c) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if ((int)blockIdx.x < a.writers) {  // (block-uniform)
        refit_body<LDS>(a, blockIdx.x, smem);
        return;
    }
    states_small_body<true, false>(smem, (int)blockIdx.x - a.writers, c.recs, c.n_obb, c.rg, c.ro, c.xyz, c.n, c.per, 0,
                                   c.md, c.valid, nullptr, nullptr);
    publish_done(a.done + blockIdx.x, a.seq);
}

// The latency path's per-thread state (StreamBufs): h_in the kernel's inputs, h_out
// [status (8 B) | pad | completion slots (at +64) | check flags (at +256) | rows], d_scr the
// segment scratch (one per workgroup) of long tracks.
struct RefitCache : StreamBufs {
    uint32_t seq = 0;
    std::vector<double> T, tin, tac;  // host side of the refit: times and samples
    std::vector<int32_t> seg;
};
constexpr size_t kRowsAt = 256;  // h_out: [status | pad | slots (<= 48 x 4 B) | flags | rows]

// What the host side of a call decides (refit_host_side): the launch's sizes.
struct RefitPlan {
    int M, R, G;     // segments, rows, the refit's workgroups
    bool lds, big;   // the solve's scratch in LDS; (else) the vertex values and coefficients in global scratch too
    // the fused check (chk): the lookahead points after the refit's inputs (h_in), their
    // flags after the completion slots (h_out); its workgroups after the refit's.  The
    // records' snapshot (and its lease: no update rewrites them) is held until the poll ends.
    SmallWorld sw{};
    int64_t nck = 0;
    int per = kSmallBlock, Gc = 0;
    size_t in_refit, rows_at;  // doubles of h_in before the check's points; bytes of h_out before the rows
};

// Step 1, the host side of the refit: the segment times (Nfabian with the host's libm, or
// the caller's), Trajectory::evaluateRange's sample recurrence into c, and the sizes.
epp_status refit_host_side(RefitCache& c, const FusedCheck* chk, const double* wp, int32_t n_wp, const double* times,
                           double v_max, double a_max, double dt, RefitPlan& p) {
    const int M = n_wp - 1;
    c.T.resize(M);
    for (int i = 0; i < M; ++i) {
        c.T[i] = times ? times[i] : nfabian(wp + 3 * i, wp + 3 * (i + 1), v_max, a_max);
        if (!(c.T[i] > 0)) {  // CHECK_GT(segment_time, 0)  impl :297
            set_error(fit_status_message(-2));
            return EPP_ERR_RUNTIME;
        }
    }
    c.tin.clear();
    c.tac.clear();
    c.seg.clear();
    if (dt > 0) {
        RangeIter it;
        it.init(c.T.data(), M);
        int sg[kRowChunk];
        double ti[kRowChunk], ta[kRowChunk];
        for (int done = 0; !done;) {
            const int n = range_produce(it, dt, kRowChunk, sg, ti, ta, done);
            c.seg.insert(c.seg.end(), sg, sg + n);
            c.tin.insert(c.tin.end(), ti, ti + n);
            c.tac.insert(c.tac.end(), ta, ta + n);
        }
    }
    const int R = (int)c.tin.size();
    const bool lds = M <= kMaxLdsSeg;
    // long tracks whose vertex values and coefficients would not fit LDS beside the rest
    // (from 276 segments: e.g. a track smoothed by "ompl" simplification) keep them in the
    // global scratch too
    const bool big = !lds && refit_lds_doubles(M, false) * sizeof(double) > kLdsBudget;
    if (refit_lds_doubles(M, lds, big) * sizeof(double) > kLdsBudget) {
        set_error("generateTrajectory: too many waypoints for one workgroup's LDS (" + std::to_string(n_wp) + ")");
        return EPP_ERR_UNSUPPORTED;
    }
    p.M = M;
    p.R = R;
    p.lds = lds;
    p.big = big;
    p.G = R ? std::min(kRefitMaxWriters, (R + kRefitRowChunk - 1) / kRefitRowChunk) : 1;
    p.nck = chk ? chk->n : 0;
    if (p.nck > 0) {
        p.sw = small_world(chk->world);
        if (p.nck > kSmallStates || p.sw.n_obb > kSmallMaxObbs) {
            set_error("checkAndGenerate: the check is not small (<= 4096 points, <= 256 OBBs)");
            return EPP_ERR_UNSUPPORTED;
        }
        p.per = small_per(p.nck);
        p.Gc = (int)((p.nck + p.per - 1) / p.per);
    }
    p.in_refit = (refit_in_doubles(n_wp, R) + 1) & ~size_t(1);  // (16-byte aligned points after it)
    p.rows_at = kRowsAt + (((size_t)p.nck + 255) & ~size_t(255));
    return EPP_OK;
}

// Step 2: the pinned input (c.h_in, sized by the caller) and the kernels' two argument
// structs (ck only with a fused check).
void refit_fill(RefitCache& c, const RefitPlan& p, const FusedCheck* chk, const double* wp, int32_t n_wp, double t0,
                const double v0[3], const double a0[3], RefitArgs& a, CheckArgs& ck) {
    const int M = p.M, R = p.R;
    double* in = c.h_in.as<double>();
    char* const h_out = c.h_out.as<char>();
    std::memcpy(in, wp, (size_t)n_wp * 24);
    for (int k = 0; k < 3; ++k) {
        in[3 * n_wp + k] = v0 ? v0[k] : 0.0;
        in[3 * n_wp + 3 + k] = a0 ? a0[k] : 0.0;
    }
    std::memcpy(in + 3 * n_wp + 6, c.T.data(), (size_t)M * 8);
    double* ins = in + 3 * n_wp + 6 + M;
    if (R) {
        std::memcpy(ins, c.tin.data(), (size_t)R * 8);
        std::memcpy(ins + R, c.tac.data(), (size_t)R * 8);
        std::memcpy(ins + 2 * R, c.seg.data(), (size_t)R * 4);
    }
    a.in = in;
    a.W = n_wp;
    a.R = R;
    a.writers = p.G;
    a.seq = next_seq(c.seq);
    a.t0 = t0;
    if (n_wp <= kRefitArgW) std::memcpy(a.small, in, (size_t)(3 * n_wp + 6 + M) * 8);
    a.info = reinterpret_cast<int64_t*>(h_out);
    a.done = reinterpret_cast<uint32_t*>(h_out + 64);
    a.out = reinterpret_cast<double*>(h_out + p.rows_at);
    a.scratch = c.d_scr;
    a.big = p.big ? 1 : 0;
    {  // the latency path solves without the refinement step: it cost 6-7 us of a ~30 us
       // call (scripts/refit_ab.py) for ~1e-10 of accuracy the sampled rows do not need
       // (rows vs the truth 6e-11 either way).  EPP_REFIT_REFINE=1: with it (A/B knob)
        static const int refine = [] {
            const char* e = std::getenv("EPP_REFIT_REFINE");
            return e && *e == '1' ? 1 : 0;
        }();
        a.refine = refine;
    }
    a.info[0] = -100;
    if (p.Gc > 0) {
        double* pts = in + p.in_refit;
        std::memcpy(pts, chk->xyz, (size_t)p.nck * 24);
        ck.recs = p.sw.recs;
        ck.n_obb = p.sw.n_obb;
        ck.per = p.per;
        ck.rg = p.sw.r_gate;
        ck.ro = p.sw.r_obst;
        ck.md = chk->min_distance;
        ck.xyz = pts;
        ck.n = p.nck;
        ck.valid = reinterpret_cast<uint8_t*>(h_out + kRowsAt);
    }
}

// Step 3: the launch, and the poll of every workgroup's completion slot.  *info: the fit's
// status (still -100: it was never written).
hipError_t refit_launch_poll(RefitCache& c, const RefitPlan& p, const RefitArgs& a, const CheckArgs& ck,
                             int64_t* info) {
    const int G = p.G, Gc = p.Gc;
    const bool lds = p.lds;
    size_t shm = refit_lds_doubles(p.M, lds, p.big) * sizeof(double);
    if (Gc > 0) {
        shm = std::max(shm, small_shm(p.sw.n_obb));
        if (lds) {
            allow_lds(k_check_refit<true>);
            hipLaunchKernelGGL(k_check_refit<true>, dim3(G + Gc), dim3(kRefitBlock), shm, c.s, a, ck);
        } else {
            allow_lds(k_check_refit<false>);
            hipLaunchKernelGGL(k_check_refit<false>, dim3(G + Gc), dim3(kRefitBlock), shm, c.s, a, ck);
        }
    } else if (lds) {
        allow_lds(k_refit<true>);
        hipLaunchKernelGGL(k_refit<true>, dim3(G), dim3(kRefitBlock), shm, c.s, a);
    } else {
        allow_lds(k_refit<false>);
        hipLaunchKernelGGL(k_refit<false>, dim3(G), dim3(kRefitBlock), shm, c.s, a);
    }
    hipError_t e = hipGetLastError();
    // wait for every workgroup's slot; slot 0's release follows the status store of the
    // same lane, so the status is visible with it
    *info = -100;
    if (e == hipSuccess) {
        const WaitResult r = wait_done(a.done, G + Gc, a.seq, c.s, 0.0);
        if (r.kind == WaitResult::kHipError) e = r.err;
        else if (r.kind != WaitResult::kDone || (*info = a.info[0]) == -100)
            e = hipErrorUnknown;  // finished without its completion words
    }
    return e;
}

}  // namespace

// poly_traj::generateTrajectory with host buffers (src/trajectory_generator.cpp:12-100).
// The host computes the segment times (estimateSegmentTimesNfabian with its libm, as the
// reference, or the caller's) and runs Trajectory::evaluateRange's sample recurrence
// (src/trajectory.cpp:81-141: exact count, times and segments); one launch of k_refit then
// solves and writes the rows straight into pinned memory; one poll of the completion slots.
// The rows are copied once, from the pinned buffer the kernel wrote into the buffer
// alloc(ctx, R) returns (the C ABI: malloc; the C++ API: the result matrix itself).
epp_status generate_trajectory_into(const double* wp, int32_t n_wp, const double* times, double v_max, double a_max,
                                    double dt, double t0, const double v0[3], const double a0[3],
                                    double* (*alloc)(void*, int64_t), void* ctx, int64_t* n_rows) {
    return check_and_generate_into(nullptr, wp, n_wp, times, v_max, a_max, dt, t0, v0, a0, alloc, ctx, n_rows);
}

epp_status check_and_generate_into(const FusedCheck* chk, const double* wp, int32_t n_wp, const double* times,
                                   double v_max, double a_max, double dt, double t0, const double v0[3],
                                   const double a0[3], double* (*alloc)(void*, int64_t), void* ctx, int64_t* n_rows) {
    if (!alloc || !n_rows || (n_wp > 0 && !wp) ||
        (chk && (!chk->world || chk->n < 0 || (chk->n > 0 && (!chk->xyz || !chk->valid))))) {
        set_error("generateTrajectory: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    *n_rows = 0;
    if (n_wp < 2) {
        set_error("At least two waypoints are required");  // trajectory_generator.cpp:24
        return EPP_ERR_INVALID_ARGUMENT;
    }
    epp_status rc = ensure_consts();
    if (rc) return rc;
    static thread_local RefitCache c;
    RefitPlan p;
    if ((rc = refit_host_side(c, chk, wp, n_wp, times, v_max, a_max, dt, p))) return rc;
    const int R = p.R;
    hipError_t e = c.bind();
    if (e == hipSuccess)  // (a new h_out zeroed: its completion slots)
        e = c.ensure((p.in_refit + 3 * (size_t)p.nck) * 8, (size_t)R * 80 + p.rows_at,
                     p.lds ? 0 : (size_t)p.G * refit_scr_doubles(p.M, p.big) * 8, true);
    if (e != hipSuccess) return buffers_error(e);
    RefitArgs a;
    CheckArgs ck;
    refit_fill(c, p, chk, wp, n_wp, t0, v0, a0, a, ck);
    int64_t info;
    e = refit_launch_poll(c, p, a, ck, &info);
    if (e != hipSuccess) {
        set_error(std::string("generateTrajectory: ") + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    if (p.Gc > 0) std::memcpy(chk->valid, c.h_out.as<char>() + kRowsAt, (size_t)p.nck);
    if (info != 0) {
        set_error(fit_status_message((int)info));
        return EPP_ERR_RUNTIME;
    }
    double* host_rows = alloc(ctx, R);
    if (!host_rows) {
        set_error("generateTrajectory: out of host memory");
        return EPP_ERR_RUNTIME;
    }
    if (R) std::memcpy(host_rows, a.out, (size_t)R * 80);
    *n_rows = R;
    return EPP_OK;
}

}  // namespace epp

#ifdef EPP_REFIT_TL
// diagnostics builds only: the last refit's phase timeline (2 workgroups x 16 stamps)
extern "C" epp_status epp_dbg_refit_tl(unsigned long long* out) {
    using namespace epp;
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_refit_tl), sizeof(g_refit_tl));
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out + 32, HIP_SYMBOL(g_refit_it), sizeof(g_refit_it));
    return e == hipSuccess ? EPP_OK : EPP_ERR_HIP;
}
#endif
