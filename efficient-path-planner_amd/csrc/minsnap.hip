// minsnap.hip — the batch stage of the minimum-snap fit for gfx950: many tracks fitted
// (k_minsnap: one 64-lane wavefront per track runs solve_track, minsnap_solve.h) and sampled
// (k_sample_count, k_sample_rows) per launch, and the two single-track launchers of
// minsnap_kernels.h.
//
// Sampling reproduces Trajectory::evaluateRange (src/trajectory.cpp:81-141) exactly:
// one lane runs the sequential `acc += dt` / segment roll-over recurrence (so sample
// times and counts are bit-identical), and the wavefront evaluates the rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "cached_ws.h"
#include "collision_common.h"
#include "minsnap_kernels.h"
#include "minsnap_solve.h"

namespace epp {
namespace {

// Batch: one workgroup (BLOCK threads) per track.  Track k owns waypoints
// [wp_off[k], wp_off[k+1]) and segments [wp_off[k]-k, wp_off[k+1]-k-1).  LDS: the segment
// scratch (when LDS) and the vertex values; else the segment scratch lives in gscratch
// at the track's first segment (Σ M x Seg::kSize doubles).
template <int BLOCK, bool LDS>
__global__ __launch_bounds__(BLOCK) void k_minsnap(const double* __restrict__ wp, const int32_t* __restrict__ wp_off,
                                                   int n_tracks, double vmax, double amax, const double* __restrict__ v0,
                                                   const double* __restrict__ a0, const double* __restrict__ times_in,
                                                   double* __restrict__ seg_times, double* __restrict__ coeffs,
                                                   int32_t* __restrict__ status, double* __restrict__ gscratch,
                                                   int refine) {
    // one dynamic LDS array (cdna_hip_programming.md Guideline 17): the error flag (16
    // bytes), the constants, then the solve's scratch
    extern __shared__ __attribute__((aligned(16))) double smem[];
    int* s_err = reinterpret_cast<int*>(smem);
    double* kc = smem + 2;
    double* sm = kc + kNC;
    stage_consts<BLOCK>(kc);
    const int track = blockIdx.x;
    if (track >= n_tracks) return;
    const int w0 = wp_off[track];
    const int W = wp_off[track + 1] - w0;
    const int M = W - 1;
    const int seg0 = w0 - track;
    if (W < 2) {
        if (threadIdx.x == 0 && status) status[track] = -1;  // std::invalid_argument
        return;
    }
    if (threadIdx.x == 0) *s_err = 0;
    double* scr = LDS ? sm : gscratch + (size_t)seg0 * Seg::kSize;
    double* dv = LDS ? sm + (size_t)M * Seg::kSize : sm;
    double* rhs = dv + (size_t)(M + 1) * 15;
    double* Tm = rhs + (size_t)(M + 1) * 12;
    __syncthreads();
    const int st = solve_track<BLOCK, LDS>(kc, wp + (size_t)w0 * 3, M, vmax, amax, v0 ? v0 + 3 * track : nullptr,
                                      a0 ? a0 + 3 * track : nullptr, times_in ? times_in + seg0 : nullptr, scr, dv, rhs,
                                      Tm, Tm + M, s_err, seg_times + seg0, coeffs + (size_t)seg0 * 30, refine != 0);
    if (threadIdx.x == 0 && status) status[track] = st;
}

// One wavefront per track: the lanes stage the segment times in LDS, lane 0 runs the
// recurrence (every step reads T[i] from LDS, not from memory).
__global__ __launch_bounds__(kWave) void k_sample_count(const double* __restrict__ seg_times,
                                                        const int32_t* __restrict__ wp_off,
                                                        int n_tracks, double dt,
                                                        int64_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) double sT[];
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    if (M < 1 || !(dt > 0)) {
        if (threadIdx.x == 0) counts[t] = 0;
        return;
    }
    const double* T = seg_times + (wp_off[t] - t);
    for (int i = threadIdx.x; i < M; i += kWave) sT[i] = T[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        RangeIter it;
        it.init(sT, M);
        counts[t] = range_count(it, dt);
    }
}

__global__ __launch_bounds__(kWave) void k_sample_rows(const double* __restrict__ seg_times,
                                                       const double* __restrict__ coeffs,
                                                       const int32_t* __restrict__ wp_off,
                                                       int n_tracks, double dt,
                                                       const double* __restrict__ t0,
                                                       const int64_t* __restrict__ row_off,
                                                       double* __restrict__ rows, int64_t cap_rows) {
    // one dynamic LDS array (Guideline 17): [T (M) | tin | tac | seg (kRowChunk each) | cnt, done]
    // lane 0 runs the sequential time recurrence for kRowChunk samples at a time, then the
    // wave evaluates them (fewer barriers / coefficient-load round trips than 64 a round)
    extern __shared__ __attribute__((aligned(16))) double smB[];  // [B (kNC block) | ...]
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int lane = threadIdx.x;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    if (M < 1 || !(dt > 0)) return;
    stage_consts<kWave>(smB);
    double* sm = smB + kNC;
    const int seg0 = wp_off[t] - t;
    double* sT = sm;
    double* s_tin = sT + ((M + 1) & ~1);
    double* s_tac = s_tin + kRowChunk;
    int* s_seg = reinterpret_cast<int*>(s_tac + kRowChunk);
    int& s_cnt = s_seg[kRowChunk];
    int& s_done = s_seg[kRowChunk + 1];
    for (int i = lane; i < M; i += kWave) sT[i] = seg_times[seg0 + i];
    const double toff = t0 ? t0[t] : 0.0;
    double* out = rows + (row_off ? row_off[t] : 0) * 10;
    RangeIter it;
    __syncthreads();
    if (lane == 0) {
        it.init(sT, M);
        s_done = 0;
    }
    int64_t base = 0;
    while (true) {
        if (lane == 0) s_cnt = range_produce(it, dt, kRowChunk, s_seg, s_tin, s_tac, s_done);
        __syncthreads();
        const int cnt = s_cnt, done = s_done;
        for (int j = lane; j < cnt && base + j < cap_rows; j += kWave) {  // (cap: single-track host path)
            const double* cs = coeffs + (size_t)(seg0 + s_seg[j]) * 30;
            const double tin = s_tin[j];
            double* row = out + (base + j) * 10;
            for (int d = 0; d < 3; ++d)
                for (int k = 0; k < 3; ++k) row[3 * d + k] = poly_eval(smB + kCB, cs + d * N, tin, k);
            row[9] = s_tac[j] + toff;  // sampling_times[i] + startTimeOffset
        }
        base += cnt;
        __syncthreads();
        if (done) break;
    }
}
// k_sample_rows's dynamic LDS (the layout above) for tracks of up to max_m segments
size_t sample_rows_shm(int max_m) { return ((size_t)kNC + ((max_m + 1) & ~1) + 3 * kRowChunk + 2) * 8; }

CachedWs g_minsnap_ws[64];

epp_status minsnap_batch(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, double v_max, double a_max,
                         const double* v0, const double* a0, const double* times_in, double* seg_times, double* coeffs,
                         int32_t* status, void* stream, const char* what, int known_m = -1) {
    if (n_tracks < 0 || (n_tracks > 0 && (!wp || !wp_offsets || !seg_times || !coeffs))) {
        set_error(std::string(what) + ": invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    epp_status st = ensure_consts();
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    int max_m = 0;
    int64_t total_m = 0;
    if (known_m >= 0) {  // (one track whose segment count the host caller knows)
        max_m = std::max(1, known_m);
        total_m = known_m;
    } else if ((st = read_offsets(wp_offsets, n_tracks, s, what, &max_m, &total_m))) {
        return st;
    }
    constexpr int kB = 64;  // one wavefront per track: the batch is throughput-bound
    // one refinement step in every track's solve (solve_track): +50 % kernel time, 10-100x
    // the accuracy on short and mixed segments (scripts/minsnap_truth_probe.py, DESIGN.md
    // section 4); EPP_MINSNAP_REFINE=0 skips it (A/B knob)
    static const int refine = [] {
        const char* e = std::getenv("EPP_MINSNAP_REFINE");
        return e && *e == '0' ? 0 : 1;
    }();
    if (max_m <= kMaxLdsSeg) {
        const size_t shm = ((size_t)max_m * Seg::kSize + vertex_doubles(max_m) + 2 + kNC) * sizeof(double);
        allow_lds(k_minsnap<kB, true>);
        hipLaunchKernelGGL((k_minsnap<kB, true>), dim3(n_tracks), dim3(kB), shm, s, wp, wp_offsets, n_tracks, v_max,
                           a_max, v0, a0, times_in, seg_times, coeffs, status, nullptr, refine);
        return launch_error(what);
    }
    // long tracks: segment scratch in a per-device workspace whose reuse by another stream
    // waits for this launch (CachedWs)
    int dev = 0;
    (void)hipGetDevice(&dev);
    CachedWs& ws = g_minsnap_ws[dev & 63];
    std::lock_guard<std::mutex> lk(ws.mu);
    const hipError_t e = ws.acquire(s, (size_t)std::max<int64_t>(total_m, 1) * Seg::kSize * sizeof(double));
    if (e != hipSuccess) {
        set_error(std::string(what) + ": workspace: " + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    const size_t shm = (vertex_doubles(max_m) + 2 + kNC) * sizeof(double);
    if (shm > kLdsBudget) {
        ws.release(s);
        set_error(std::string(what) + ": a track has too many waypoints for one workgroup's LDS (" +
                  std::to_string(max_m + 1) + ")");
        return EPP_ERR_UNSUPPORTED;
    }
    allow_lds(k_minsnap<kB, false>);
    hipLaunchKernelGGL((k_minsnap<kB, false>), dim3(n_tracks), dim3(kB), shm, s, wp, wp_offsets, n_tracks, v_max, a_max,
                       v0, a0, times_in, seg_times, coeffs, status, static_cast<double*>(ws.buf), refine);
    st = launch_error(what);
    ws.release(s);
    return st;
}

}  // namespace

// The batch fits' segment scratch of a device (minsnap_constrained.hip shares it).
CachedWs& minsnap_workspace(int dev) { return g_minsnap_ws[dev & 63]; }

// The track offsets of a batch (they live on the device; the launchers need the largest
// segment count to size LDS and the total for the global scratch; minsnap_kernels.h).
epp_status read_offsets(const int32_t* d_off, int n_tracks, hipStream_t s, const char* what, int* max_m,
                        int64_t* total_m) {
    std::vector<int32_t> off(n_tracks + 1);
    hipError_t e = hipMemcpyAsync(off.data(), d_off, off.size() * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error(std::string(what) + ": reading track offsets: " + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    int m = 1;
    int64_t tot = 0;
    for (int t = 0; t < n_tracks; ++t) {
        const int mt = off[t + 1] - off[t] - 1;
        m = std::max(m, mt);
        tot += std::max(0, mt);
    }
    *max_m = m;
    if (total_m) *total_m = tot;
    return EPP_OK;
}

epp_status launch_minsnap_track(const double* wp, const int32_t* wp_off, int M, double v_max, double a_max,
                                const double* v0, const double* a0, double* seg_times, double* coeffs,
                                int32_t* status, hipStream_t st, const char* what) {
    return minsnap_batch(wp, wp_off, 1, v_max, a_max, v0, a0, nullptr, seg_times, coeffs, status, st, what, M);
}

epp_status launch_sample_rows_track(const double* seg_times, const double* coeffs, const int32_t* wp_off, int M,
                                    double dt, const double* t0, double* rows, int64_t cap_rows, hipStream_t st,
                                    const char* what) {
    const epp_status rc = ensure_consts();
    if (rc) return rc;
    hipLaunchKernelGGL(k_sample_rows, dim3(1), dim3(kWave), sample_rows_shm(M), st, seg_times, coeffs, wp_off, 1, dt,
                       t0, (const int64_t*)nullptr, rows, cap_rows);
    return launch_error(what);
}

}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_minsnap_batch(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, double v_max,
                             double a_max, const double* v0, const double* a0, double* seg_times, double* coeffs,
                             int32_t* status, void* stream) {
    return minsnap_batch(wp, wp_offsets, n_tracks, v_max, a_max, v0, a0, nullptr, seg_times, coeffs, status, stream,
                         "epp_minsnap_batch");
}

epp_status epp_minsnap_batch_times(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, const double* v0,
                                   const double* a0, const double* seg_times_in, double* coeffs, int32_t* status,
                                   void* stream) {
    if (n_tracks > 0 && !seg_times_in) {
        set_error("epp_minsnap_batch_times: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    // the kernel copies the caller's times to seg_times: in place is fine (same index)
    return minsnap_batch(wp, wp_offsets, n_tracks, 0.0, 0.0, v0, a0, seg_times_in, const_cast<double*>(seg_times_in),
                         coeffs, status, stream, "epp_minsnap_batch_times");
}

epp_status epp_sample_count(const double* seg_times, const int32_t* wp_offsets, int32_t n_tracks, double dt,
                            int64_t* row_counts, void* stream) {
    if (n_tracks < 0 || (n_tracks > 0 && (!seg_times || !wp_offsets || !row_counts))) {
        set_error("epp_sample_count: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    int max_m = 0;
    epp_status st = read_offsets(wp_offsets, n_tracks, (hipStream_t)stream, "epp_sample_count", &max_m, nullptr);
    if (st) return st;
    hipLaunchKernelGGL(k_sample_count, dim3(n_tracks), dim3(kWave), (size_t)(max_m + 2) * 8, (hipStream_t)stream,
                       seg_times, wp_offsets, n_tracks, dt, row_counts);
    return launch_error("epp_sample_count");
}

epp_status epp_sample_batch(const double* seg_times, const double* coeffs, const int32_t* wp_offsets, int32_t n_tracks,
                            double dt, const double* t0, const int64_t* row_offsets, double* rows, void* stream) {
    if (n_tracks < 0 || (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !row_offsets || !rows))) {
        set_error("epp_sample_batch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    epp_status st = ensure_consts();
    if (st) return st;
    int max_m = 0;
    if ((st = read_offsets(wp_offsets, n_tracks, (hipStream_t)stream, "epp_sample_batch", &max_m, nullptr))) return st;
    hipLaunchKernelGGL(k_sample_rows, dim3(n_tracks), dim3(kWave), sample_rows_shm(max_m), (hipStream_t)stream,
                       seg_times, coeffs, wp_offsets, n_tracks, dt, t0, row_offsets, rows, (int64_t)INT64_MAX);
    return launch_error("epp_sample_batch");
}

}  // extern "C"
