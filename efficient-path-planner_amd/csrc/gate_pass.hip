// gate_pass.hip — which gates straight edges cross (epp_gates_crossed) and which gates, in
// order, the chords of fitted tracks pass, and when (epp_traj_gate_pass_batch), straight from
// the tracks' coefficients (gfx950).  The predicate is gate_pass.h's:
//
//   OnlineTrajGenerator::checkGatePassed  src/OnlineTrajGenerator.cpp:228-256, which
//   updateGatePos (:123-226) calls for one gate over the rows of one sampled trajectory.
//
// k_gates_crossed: one edge per lane, the frame table in LDS (every lane of a wave reads the
// same frame: a broadcast read), a loop over the gates, one 64-bit mask per edge.
//
// k_traj_gates: the walk of traj_walk.h with the check TcGates.  Ordered passage of a track
// with chords j = row j -> row j + 1: c_-1 = 0, c_g = the smallest j >= c_g-1 whose chord
// crosses gate g; the first gate without one and every later gate are unpassed.  The check
// never posts, so every chunk of every track is walked.
#include <algorithm>
#include <cmath>

#include "gate_pass.h"
#include "launch_helpers.h"
#include "traj_walk.h"

namespace epp {
namespace {

constexpr int kGcBlock = 256;

__global__ __launch_bounds__(kGcBlock) void k_gates_crossed(const double* __restrict__ gates, int n_gates,
                                                            double half_edge, const double* __restrict__ s1,
                                                            const double* __restrict__ s2, int64_t n,
                                                            uint64_t* __restrict__ mask) {
    __shared__ double fr[kMaxGates * kGateDoubles];
    for (int k = threadIdx.x; k < n_gates * kGateDoubles; k += kGcBlock) fr[k] = gates[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kGcBlock + threadIdx.x;
    if (i >= n) return;
    const double ax = s1[3 * i], ay = s1[3 * i + 1], az = s1[3 * i + 2];
    const double bx = s2[3 * i], by = s2[3 * i + 1], bz = s2[3 * i + 2];
    uint64_t m = 0;
    for (int g = 0; g < n_gates; ++g)
        m |= (uint64_t)gate_cross(fr + g * kGateDoubles, half_edge, ax, ay, az, bx, by, bz).crossed << g;
    mask[i] = m;
}

// What k_traj_gates keeps in LDS behind TcShared: the frame table, staged once per workgroup,
// and the passes of the track being walked, which the checking wave records and writes out.
struct TgShared {
    double frames[kMaxGates * kGateDoubles];
    long long chord[kMaxGates];
    double time[kMaxGates];
    double off[kMaxGates][2];
};

struct TgOut {
    double* offset;     // n_tracks x n_gates x 2, may be NULL
    int32_t* n_passed;  // n_tracks
};

constexpr int kTgOwn = kRowChunk / kTcCheckers;  // samples a lane owns in a full chunk

// The chords as TcChords (trajcheck.hip) takes them: a checking lane owns G = ceil(cnt / 64)
// consecutive samples of the chunk and the chords that END at them; the chord into its first
// sample starts at the last sample of the lane before it, handed up by a lane shift, and lane
// 0 takes the previous chunk's last position, carried in registers of wave 1 with that row's
// time.  Per owned chord the lane builds the mask of the gates >= the track's next gate that
// the chord crosses.  Then the wave resolves the order: while some lane owns a chord >= the
// current one with the next gate's bit set, a ballot picks the lowest such lane (lanes own
// ascending chords), its lowest such chord is broadcast and becomes the current one, the lane
// records the pass and the next gate advances -- the same chord may pass it too.  The record
// (chord, time, offsets) goes to LDS, written and at the track's end read by wave 1 alone:
// no barrier beyond the walk's, nothing for thread 0 to do.
struct TcGates {
    TgShared& o;
    int n_gates;
    double half_edge;
    TgOut out;
    double cx, cy, cz, ctac;  // wave 1: the previous chunk's last position and time
    long long cur;            // wave 1: c_{next - 1}
    int next;                 // wave 1: the first gate not passed yet
    __device__ __forceinline__ void reset() {
        cx = cy = cz = ctac = 0.0;
        cur = 0;
        next = 0;
    }
    __device__ __forceinline__ void begin() { reset(); }
    __device__ __forceinline__ void keep(const TcShared&, int) {}
    __device__ __forceinline__ void check(TcShared& s, int b, int cnt, int64_t base, int lane,
                                          const double* __restrict__ coeffs, int seg0) {
        const int G = (cnt + kTcCheckers - 1) / kTcCheckers;  // <= kTgOwn
        const int j0 = lane * G;
        const int j1 = min(j0 + G, cnt);
        const bool has = j0 < cnt;
        double l[3] = {0.0, 0.0, 0.0};  // the lane's last sample
        if (has) tc_pos(s, b, j1 - 1, coeffs, seg0, l);
        // (whole wave; a lane without samples hands up zeros, which only a lane without samples receives)
        double q0[3] = {__shfl_up(l[0], 1), __shfl_up(l[1], 1), __shfl_up(l[2], 1)};
        if (lane == 0) {
            q0[0] = cx;
            q0[1] = cy;
            q0[2] = cz;
        }
        const double ptac = ctac;
        cx = __shfl(l[0], kTcCheckers - 1);  // (a full chunk: sample kRowChunk - 1; else unused)
        cy = __shfl(l[1], kTcCheckers - 1);
        cz = __shfl(l[2], kTcCheckers - 1);
        ctac = s.tac[b][kRowChunk - 1];
        uint64_t m[kTgOwn];
        double q[3] = {q0[0], q0[1], q0[2]};
#pragma unroll
        for (int k = 0; k < kTgOwn; ++k) {
            m[k] = 0;
            const int j = j0 + k;
            if (j < j1) {
                double e[3] = {l[0], l[1], l[2]};
                if (j < j1 - 1) tc_pos(s, b, j, coeffs, seg0, e);
                if ((base | j) != 0)  // (row 0 ends no chord)
                    for (int g = next; g < n_gates; ++g)
                        m[k] |= (uint64_t)gate_cross(o.frames + g * kGateDoubles, half_edge, q[0], q[1], q[2], e[0],
                                                     e[1], e[2]).crossed << g;
                q[0] = e[0];
                q[1] = e[1];
                q[2] = e[2];
            }
        }
        while (next < n_gates) {  // (wave-uniform)
            int kk = kTgOwn;      // the lane's lowest chord >= cur that crosses gate `next`
#pragma unroll
            for (int k = kTgOwn - 1; k >= 0; --k)
                if (((m[k] >> next) & 1u) && base + j0 + k - 1 >= cur) kk = k;
            const unsigned long long vote = __ballot(kk < kTgOwn);
            if (!vote) break;
            const int src = __ffsll(vote) - 1;
            const int j = __shfl(j0 + kk, src);  // the chord's end sample in the half
            if (lane == src) {
                double a[3] = {q0[0], q0[1], q0[2]}, e[3];
                if (kk > 0) tc_pos(s, b, j - 1, coeffs, seg0, a);
                tc_pos(s, b, j, coeffs, seg0, e);
                const GateCross r =
                    gate_cross(o.frames + next * kGateDoubles, half_edge, a[0], a[1], a[2], e[0], e[1], e[2]);
                // the two rows' time columns as epp_sample_batch writes them with t0 == NULL
                const double t0 = (j > 0 ? s.tac[b][j - 1] : ptac) + 0.0, t1 = s.tac[b][j] + 0.0;
                o.chord[next] = base + j - 1;
                o.time[next] = t0 + r.u() * (t1 - t0);
                o.off[next][0] = r.mx;
                o.off[next][1] = r.mz;
            }
            cur = base + j - 1;
            ++next;
        }
    }
    __device__ __forceinline__ int row(int f) const { return f; }                           // (never posted:
    __device__ __forceinline__ double time(const TcShared&, int, int) const { return 0.0; }  //  never asked)
    __device__ __forceinline__ void posted(const TcShared&, int, int, const double* __restrict__, int) {}
    __device__ __forceinline__ void end(int t, int tid, bool walked, int64_t, double, int64_t* __restrict__ chord,
                                        double* __restrict__ time) {
        if (tid < 64) return;  // (wave-uniform: wave 1 holds the passes)
        if (!walked) reset();  // no segment, no row
        const int g = tid - 64;
        // (the records were written in check(), before the walk's barrier of that chunk; the next
        // track's are written after its walk's first barriers)
        if (g < n_gates) {
            const bool passed = g < next;
            const size_t i = (size_t)t * n_gates + g;
            chord[i] = passed ? o.chord[g] : -1;
            if (time) time[i] = passed ? o.time[g] : -1.0;
            if (out.offset) {
                out.offset[2 * i] = passed ? o.off[g][0] : NAN;
                out.offset[2 * i + 1] = passed ? o.off[g][1] : NAN;
            }
        }
        if (g == 0) out.n_passed[t] = next;
        reset();
    }
};

__global__ __launch_bounds__(kTcBlock) void k_traj_gates(const double* __restrict__ gates, int n_gates,
                                                         double half_edge, const double* __restrict__ seg_times,
                                                         const double* __restrict__ coeffs,
                                                         const int32_t* __restrict__ wp_off, int n_tracks, double dt,
                                                         TgOut out, int64_t* __restrict__ chord,
                                                         double* __restrict__ time) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    TgShared& o = *reinterpret_cast<TgShared*>(lds + kTcSharedBytes);
    for (int k = threadIdx.x; k < n_gates * kGateDoubles; k += kTcBlock) o.frames[k] = gates[k];
    __syncthreads();
    TcGates chk{o, n_gates, half_edge, out};
    chk.reset();
    tc_walk(*reinterpret_cast<TcShared*>(lds), seg_times, coeffs, wp_off, n_tracks, dt, chord, time, chk);
}

bool gates_ok(int32_t n_gates, double half_edge) {
    return n_gates >= 0 && n_gates <= kMaxGates && half_edge >= 0.0 && std::isfinite(half_edge);
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_gates_crossed(const double* gates, int32_t n_gates, double half_edge, const double* s1, const double* s2,
                             int64_t n, uint64_t* mask, void* stream) {
    const int64_t groups = n > 0 ? (n + kGcBlock - 1) / kGcBlock : 0;
    if (!gates_ok(n_gates, half_edge) || n < 0 || groups > INT_MAX ||
        (n > 0 && (!s1 || !s2 || !mask || (n_gates > 0 && !gates)))) {
        set_error("epp_gates_crossed: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    hipLaunchKernelGGL(k_gates_crossed, dim3((unsigned)groups), dim3(kGcBlock), 0, (hipStream_t)stream, gates,
                       (int)n_gates, half_edge, s1, s2, n, mask);
    return launch_error("epp_gates_crossed");
}

epp_status epp_traj_gate_pass_batch(const double* gates, int32_t n_gates, double half_edge, const double* seg_times,
                                    const double* coeffs, const int32_t* wp_offsets, int32_t n_tracks, double dt,
                                    int64_t* chord, double* time, double* offset, int32_t* n_passed, void* stream) {
    if (!gates_ok(n_gates, half_edge) || n_tracks < 0 || !(dt > 0) || !std::isfinite(dt) ||
        (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !n_passed || (n_gates > 0 && (!gates || !chord))))) {
        set_error("epp_traj_gate_pass_batch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    if (n_gates == 0) {  // nothing to pass
        if (hipMemsetAsync(n_passed, 0, (size_t)n_tracks * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
            set_error("epp_traj_gate_pass_batch: memset failed");
            return EPP_ERR_HIP;
        }
        return EPP_OK;
    }
    const uint32_t shm = kTcSharedBytes + (uint32_t)sizeof(TgShared);
    // persistent grid: as many workgroups as stay resident (trajcheck.hip: 8 per CU by registers, fewer by LDS)
    const int per_cu = std::max(1, std::min<int>(8, (int)((160u * 1024u) / shm)));
    const int grid = (int)std::min<int64_t>(n_tracks, (int64_t)cu_count() * per_cu);
    hipLaunchKernelGGL(k_traj_gates, dim3(grid), dim3(kTcBlock), shm, (hipStream_t)stream, gates, (int)n_gates,
                       half_edge, seg_times, coeffs, wp_offsets, (int)n_tracks, dt, TgOut{offset, n_passed}, chord, time);
    return launch_error("epp_traj_gate_pass_batch");
}

}  // extern "C"
