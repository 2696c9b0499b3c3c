// minsnap_constrained.hip — the batch fit with the caller's constraints for gfx950: the end
// vertices' four derivatives and any derivatives of inner waypoints prescribed
// (k_minsnap_constrained: one 64-lane wavefront per track runs solve_track under the
// VertexPins policy, minsnap_solve.h), and the single-track launcher of minsnap_kernels.h.
//
// Reference: Vertex::addConstraint / makeStartOrEnd (src/vertex.cpp:30-60, :146-170) and
// PolynomialOptimization<10>::setupFromVertices, which takes any such vertex set; the
// reference's generateTrajectory (external/poly_traj/src/trajectory_generator.cpp:28-50) only
// ever builds one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "cached_ws.h"
#include "collision_common.h"
#include "minsnap_kernels.h"
#include "minsnap_solve.h"

namespace epp {
namespace {

// The mask bytes of a track of M segments in LDS, after the solve's vertex data (doubles, so
// that what follows stays 16-byte aligned: Guideline 17).
__host__ __device__ constexpr size_t mask_doubles(int M) { return (((size_t)M + 1 + 15) / 16) * 2; }

// Batch: one workgroup (BLOCK threads) per track, the layout of k_minsnap (minsnap.hip).
// fixed_mask: one byte per waypoint; fixed_val: 12 doubles per waypoint, (k-1) * 3 + d.  LDS:
// the segment scratch (when LDS), the vertex values, the track's mask bytes with the two end
// vertices' set to 0xF.  A mask bit above bit 3 at an inner waypoint, or a non-finite value in
// a slot that is used: status -4, nothing else written.
template <int BLOCK, bool LDS>
__global__ __launch_bounds__(BLOCK) void k_minsnap_constrained(
    const double* __restrict__ wp, const int32_t* __restrict__ wp_off, int n_tracks, double vmax, double amax,
    const double* __restrict__ times_in, const uint8_t* __restrict__ fixed_mask, const double* __restrict__ fixed_val,
    double* __restrict__ seg_times, double* __restrict__ coeffs, int32_t* __restrict__ status,
    double* __restrict__ gscratch, int refine) {
    // one dynamic LDS array (cdna_hip_programming.md Guideline 17): the error flag (16
    // bytes), the constants, then the solve's scratch and the mask bytes
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
    uint8_t* s_mask = reinterpret_cast<uint8_t*>(Tm + M + kXch);
    const uint8_t* gm = fixed_mask + w0;
    const double* gv = fixed_val + (size_t)w0 * 12;
    int bad = 0;
    for (int v = threadIdx.x; v <= M; v += BLOCK) {
        const uint8_t mk = (v == 0 || v == M) ? 0xF : gm[v];  // makeStartOrEnd: all four
        bad |= (mk & 0xF0) != 0;
        s_mask[v] = mk & 0xF;
    }
    for (int e = threadIdx.x; e < (M + 1) * 12; e += BLOCK) {
        const int v = e / 12, k1 = (e % 12) / 3;
        const uint8_t mk = (v == 0 || v == M) ? 0xF : gm[v];
        // (finite: neither NaN nor infinite; a slot whose bit is clear is not read)
        if ((mk >> k1) & 1) bad |= !(fabs(gv[e]) <= 1.7976931348623157e308);
    }
    if (__syncthreads_or(bad)) {
        if (threadIdx.x == 0 && status) status[track] = -4;
        return;
    }
    const VertexPins pins{s_mask, gv};
    const int st = solve_track<BLOCK, LDS, VertexPins>(kc, wp + (size_t)w0 * 3, M, vmax, amax, nullptr, nullptr,
                                                         times_in ? times_in + seg0 : nullptr, scr, dv, rhs, Tm, Tm + M,
                                                         s_err, seg_times + seg0, coeffs + (size_t)seg0 * 30,
                                                         refine != 0, pins);
    if (threadIdx.x == 0 && status) status[track] = st;
}

epp_status minsnap_batch_constrained(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, double v_max,
                                     double a_max, const double* times_in, const uint8_t* fixed_mask,
                                     const double* fixed_val, double* seg_times, double* coeffs, int32_t* status,
                                     void* stream, const char* what, int known_m = -1) {
    if (n_tracks < 0 ||
        (n_tracks > 0 && (!wp || !wp_offsets || !seg_times || !coeffs || !fixed_mask || !fixed_val))) {
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
    constexpr int kB = 64;  // one wavefront per track, as k_minsnap
    // the refinement step of epp_minsnap_batch, under its knob (minsnap.hip)
    static const int refine = [] {
        const char* e = std::getenv("EPP_MINSNAP_REFINE");
        return e && *e == '0' ? 0 : 1;
    }();
    if (max_m <= kMaxLdsSeg) {
        const size_t shm =
            ((size_t)max_m * Seg::kSize + vertex_doubles(max_m) + mask_doubles(max_m) + 2 + kNC) * sizeof(double);
        allow_lds(k_minsnap_constrained<kB, true>);
        hipLaunchKernelGGL((k_minsnap_constrained<kB, true>), dim3(n_tracks), dim3(kB), shm, s, wp, wp_offsets,
                           n_tracks, v_max, a_max, times_in, fixed_mask, fixed_val, seg_times, coeffs, status, nullptr,
                           refine);
        return launch_error(what);
    }
    // long tracks: segment scratch in the batch fit's per-device workspace (CachedWs)
    int dev = 0;
    (void)hipGetDevice(&dev);
    CachedWs& ws = minsnap_workspace(dev);
    std::lock_guard<std::mutex> lk(ws.mu);
    const hipError_t e = ws.acquire(s, (size_t)std::max<int64_t>(total_m, 1) * Seg::kSize * sizeof(double));
    if (e != hipSuccess) {
        set_error(std::string(what) + ": workspace: " + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    const size_t shm = (vertex_doubles(max_m) + mask_doubles(max_m) + 2 + kNC) * sizeof(double);
    if (shm > kLdsBudget) {
        ws.release(s);
        set_error(std::string(what) + ": a track has too many waypoints for one workgroup's LDS (" +
                  std::to_string(max_m + 1) + ")");
        return EPP_ERR_UNSUPPORTED;
    }
    allow_lds(k_minsnap_constrained<kB, false>);
    hipLaunchKernelGGL((k_minsnap_constrained<kB, false>), dim3(n_tracks), dim3(kB), shm, s, wp, wp_offsets, n_tracks,
                       v_max, a_max, times_in, fixed_mask, fixed_val, seg_times, coeffs, status,
                       static_cast<double*>(ws.buf), refine);
    st = launch_error(what);
    ws.release(s);
    return st;
}

}  // namespace

epp_status launch_minsnap_constrained_track(const double* wp, const int32_t* wp_off, int M, double v_max, double a_max,
                                            const double* times_in, const uint8_t* fixed_mask,
                                            const double* fixed_val, double* seg_times, double* coeffs,
                                            int32_t* status, hipStream_t st, const char* what) {
    return minsnap_batch_constrained(wp, wp_off, 1, v_max, a_max, times_in, fixed_mask, fixed_val, seg_times, coeffs,
                                     status, st, what, M);
}

}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_minsnap_batch_constrained(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, double v_max,
                                         double a_max, const double* seg_times_in, const uint8_t* fixed_mask,
                                         const double* fixed_val, double* seg_times, double* coeffs, int32_t* status,
                                         void* stream) {
    // (caller times: the kernel copies them to seg_times; in place is fine, same index)
    return minsnap_batch_constrained(wp, wp_offsets, n_tracks, v_max, a_max, seg_times_in, fixed_mask, fixed_val,
                                     seg_times, coeffs, status, stream, "epp_minsnap_batch_constrained");
}

}  // extern "C"
