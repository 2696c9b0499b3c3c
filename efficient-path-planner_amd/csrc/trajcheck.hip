// trajcheck.hip — first collision of fitted trajectories, straight from their coefficients
// (gfx950).
//
//   PathPlanner::checkTrajectoryValidity  src/PathPlanner.cpp:267-280, per track, over the rows
//   Trajectory::evaluateRange(0, max_time, dt)  src/trajectory.cpp:81-141 would produce, with
//   World::checkPointValidity(p, minDistance)   src/World.cpp:106-128
//
// One launch, no row written: the answer per track is the index (and time) of the first row
// whose position fails, exactly what epp_sample_batch followed by epp_check_states_mindist
// gives.  The pieces are the sampler's own (traj_sample.h: the time recurrence and the fused
// Horner) and the state checks' own (collision_common.h: classify + pair_hit<true>), so the
// sample times, positions and booleans are the same bits.
//
// Shape: persistent workgroups of 2 waves, each taking tracks blockIdx.x, + gridDim.x, ...
// The time recurrence is sequential: thread 0 runs it kRowChunk samples at a time into one
// half of a double buffer in LDS (time in segment, time, segment) while wave 1 evaluates and
// checks the other half, a sample per lane and round.  A failing lane posts its sample's
// index with an LDS min; after the chunk's barrier the lowest one, if any, is the track's
// answer and the workgroup moves on, so an early collision costs at most one chunk of
// look-ahead.  The launch is bound by the recurrence, so what counts
// is how many of them run at once: two waves per workgroup (one checking wave keeps up with
// the recurrence) let ~7 workgroups share a CU; with four waves (three checking) 4 did and
// the launch took 1.5 times as long.  The world's front (occupancy masks, cell starts) is
// staged in LDS once per workgroup when it is small; the cell lists and the OBB table are
// read through L1 / L2 (consecutive samples of a track fall into the same few cells).
#include <climits>
#include <cmath>

#include "collision_common.h"
#include "traj_sample.h"

namespace epp {
namespace {

constexpr int kTcBlock = 128;
constexpr int kTcCheckers = kTcBlock - 64;  // lanes of wave 1
// Segment times staged in LDS (the tracks epp_minsnap_batch fits in LDS); a longer track's
// recurrence reads them through L2: one read per segment either way.
constexpr int kTcSegLds = 40;
// The world's front is staged in LDS up to this size (the grid has ~2 cells per OBB, 12 B
// each: worlds up to ~1000 OBBs); a larger one is read through L2.
constexpr uint32_t kTcFrontLds = 24 * 1024;

struct TcShared {
    double tin[2][kRowChunk];  // time in the segment
    double tac[2][kRowChunk];  // time from the start of the track
    int seg[2][kRowChunk];
    double T[kTcSegLds];
    int cnt[2];   // samples in the half
    int done[2];  // the recurrence ended in (or right after) the half
    int first[2]; // lowest failing sample of the half (INT_MAX: none), reset when the half is produced
};
constexpr uint32_t kTcSharedBytes = (sizeof(TcShared) + 15) & ~15u;

// The next (up to) kRowChunk samples of the recurrence into half b: k_sample_rows' loop.
// Also clears the half's result word, so each half carries its own from production to the
// read after its check.
__device__ __forceinline__ void tc_produce(RangeIter& it, TcShared& s, int b, double dt) {
    int c = 0, done = 0;
    int seg;
    double tin, tac, tin8[8], tac8[8];
    while (c < kRowChunk) {
        if (c + 8 <= kRowChunk && it.fast8(dt, tin8, tac8)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                s.seg[b][c + k] = it.i;
                s.tin[b][c + k] = tin8[k];
                s.tac[b][c + k] = tac8[k];
            }
            c += 8;
            continue;
        }
        if (!it.next(seg, tin, tac)) {
            done = 1;
            break;
        }
        s.seg[b][c] = seg;
        s.tin[b][c] = tin;
        s.tac[b][c] = tac;
        ++c;
        it.advance(dt);
    }
    s.cnt[b] = c;
    s.done[b] = done;
    s.first[b] = INT_MAX;
}

template <bool STAGE>
__global__ __launch_bounds__(kTcBlock) void k_traj_check(WorldView w, const double* __restrict__ seg_times,
                                                         const double* __restrict__ coeffs,
                                                         const int32_t* __restrict__ wp_off, int n_tracks, double dt,
                                                         double md, int64_t* __restrict__ first_invalid,
                                                         double* __restrict__ first_time, uint32_t stage_bytes) {
    // one dynamic LDS array (Guideline 17): [TcShared | the world's front (STAGE)]
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    TcShared& s = *reinterpret_cast<TcShared*>(lds);
    const unsigned char* front = STAGE ? stage_world(w, lds + kTcSharedBytes, stage_bytes) : w.blob;
    const Acc a = make_acc(front, w.blob, w);
    const int tid = threadIdx.x;
    const bool producer = tid < 64;  // wave 0 (its lane 0 runs the recurrence)
    RangeIter it;                    // (thread 0's)
    for (int t = blockIdx.x; t < n_tracks; t += gridDim.x) {
        const int w0 = wp_off[t];
        const int M = wp_off[t + 1] - w0 - 1;
        int64_t res = -1;  // no row fails (also: no segment, no row: the reference loop returns true)
        double rtime = -1.0;
        if (M >= 1) {  // (workgroup-uniform)
            const int seg0 = w0 - t;
            const double* Tg = seg_times + seg0;
            const bool t_lds = M <= kTcSegLds;
            __syncthreads();  // the previous track's reads of s are over
            if (t_lds)
                for (int i = tid; i < M; i += kTcBlock) s.T[i] = Tg[i];
            __syncthreads();
            if (tid == 0) {
                it.init(t_lds ? s.T : Tg, M);
                tc_produce(it, s, 0, dt);
            }
            __syncthreads();
            int64_t base = 0;
            int b = 0;
            // One barrier per chunk.  Ordering of the LDS accesses around it, for half b checked
            // in this iteration and half b ^ 1 produced in it:
            //  - everything of half b (samples, cnt, done, first = INT_MAX) was written by thread 0
            //    before the previous barrier; this iteration only the checkers' atomicMin touches
            //    first[b], before the barrier, and every thread reads first[b] after it;
            //  - thread 0 writes half b ^ 1 (first[b ^ 1] included) before the barrier; its last
            //    readers read it before the previous barrier, or after it only first[b ^ 1],
            //    which then held INT_MAX (a smaller value ended the track) -- the value written;
            //  - the next iteration's checkers post to first[b ^ 1], never to the word a slow
            //    wave may still be reading, so both waves take the same decision;
            //  - a track's end is followed by the next track's first barrier before any write.
            for (;;) {
                const int cnt = s.cnt[b], done = s.done[b];
                if (producer) {
                    if (tid == 0 && !done) tc_produce(it, s, b ^ 1, dt);  // the next chunk meanwhile
                } else {
                    for (int j = tid - 64; j < cnt; j += kTcCheckers) {
                        const double* cs = coeffs + (size_t)(seg0 + s.seg[b][j]) * (3 * kPolyCoeffs);
                        const double tin = s.tin[b][j];
                        const double px = poly_eval_pos(cs, tin);
                        const double py = poly_eval_pos(cs + kPolyCoeffs, tin);
                        const double pz = poly_eval_pos(cs + 2 * kPolyCoeffs, tin);
                        if (!state_valid_scalar<true>(a, w, px, py, pz, false, md)) {
                            atomicMin(&s.first[b], j);  // (a lane's samples ascend: its first failure is its lowest)
                            break;
                        }
                    }
                }
                __syncthreads();
                const int f = s.first[b];
                if (f != INT_MAX) {
                    res = base + f;
                    rtime = s.tac[b][f] + 0.0;  // epp_sample_batch's time column with t0 == NULL
                    break;
                }
                if (done) break;
                base += cnt;
                b ^= 1;
            }
        }
        if (tid == 0) {
            first_invalid[t] = res;
            if (first_time) first_time[t] = rtime;
        }
    }
}

// ---- k_traj_sweep: the chords between consecutive rows ---------------------------------
//   World::checkRayValid(p_j, p_j+1, canPassGate)  src/World.cpp:130-162, for the rows p_j of
//   Trajectory::evaluateRange(0, max_time, dt); the answer per track is the lowest j whose
//   chord fails: epp_sample_batch + epp_check_motions (mode 0) on consecutive rows.
//
// k_traj_check's shape (thread 0 runs the recurrence a chunk ahead, wave 1 checks the other
// half, one barrier per chunk).  A checking lane takes G = ceil(cnt / 64) consecutive samples
// of the chunk (8 of a full one) and tests the chords that END at them, so every chord has one
// owner: the chord into a lane's first sample starts at the last sample of the lane before
// it, which that lane evaluates first and hands up (one ds_bpermute shift per coordinate);
// lane 0 takes the previous chunk's last position, carried in a register of wave 1 (lane
// 63's, broadcast).  Every position is evaluated once; the track's first row ends no chord.
// The ray test is ray_valid (collision_common.h), the generic motion kernel's scalar walk: it
// reads cell starts, cell lists, meta words and the SoA table; everything before the table is
// staged in LDS when it fits (kTsWorldLds), else only the front, else nothing.
// LDS result word of a half: the lowest failing chord's END sample in the half (0: the chord
// from the previous chunk); its time is the START row's, which for 0 lies in the half the
// producer is overwriting: thread 0 keeps it (prev_tac) before it produces.
constexpr uint32_t kTsWorldLds = 24 * 1024;

// STAGE: 0 nothing staged, 1 the front (cell starts), 2 the blob up to the SoA table (cell
// starts, cell lists, meta words)
template <int STAGE>
__global__ __launch_bounds__(kTcBlock) void k_traj_sweep(WorldView w, const double* __restrict__ seg_times,
                                                         const double* __restrict__ coeffs,
                                                         const int32_t* __restrict__ wp_off, int n_tracks, double dt,
                                                         int can_pass, int64_t* __restrict__ first_invalid,
                                                         double* __restrict__ first_time, uint32_t stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    TcShared& s = *reinterpret_cast<TcShared*>(lds);
    const unsigned char* staged = STAGE ? stage_world(w, lds + kTcSharedBytes, stage_bytes) : w.blob;
    Acc a = make_acc(staged, w.blob, w);
    if (STAGE == 2) {
        a.meta = reinterpret_cast<const uint32_t*>(staged + w.off_meta);
        a.co = reinterpret_cast<const uint16_t*>(staged + w.off_cell_obb);
    }
    const int tid = threadIdx.x;
    const bool producer = tid < 64;
    const bool cp = can_pass != 0;
    RangeIter it;  // (thread 0's)
    for (int t = blockIdx.x; t < n_tracks; t += gridDim.x) {
        const int w0 = wp_off[t];
        const int M = wp_off[t + 1] - w0 - 1;
        int64_t res = -1;  // no chord fails (also: fewer than two rows)
        double rtime = -1.0;
        if (M >= 1) {  // (workgroup-uniform)
            const int seg0 = w0 - t;
            const double* Tg = seg_times + seg0;
            const bool t_lds = M <= kTcSegLds;
            __syncthreads();  // the previous track's reads of s are over
            if (t_lds)
                for (int i = tid; i < M; i += kTcBlock) s.T[i] = Tg[i];
            __syncthreads();
            if (tid == 0) {
                it.init(t_lds ? s.T : Tg, M);
                tc_produce(it, s, 0, dt);
            }
            __syncthreads();
            int64_t base = 0;
            int b = 0;
            double cx = 0.0, cy = 0.0, cz = 0.0;  // wave 1: the previous chunk's last position
            double prev_tac = 0.0;                // thread 0: the previous chunk's last time
            auto pos = [&](int j, double (&p)[3]) {
                const double* cs = coeffs + (size_t)(seg0 + s.seg[b][j]) * (3 * kPolyCoeffs);
                const double tin = s.tin[b][j];
                p[0] = poly_eval_pos(cs, tin);
                p[1] = poly_eval_pos(cs + kPolyCoeffs, tin);
                p[2] = poly_eval_pos(cs + 2 * kPolyCoeffs, tin);
            };
            // (the barrier and the ordering of the LDS accesses around it: as in k_traj_check)
            for (;;) {
                const int cnt = s.cnt[b], done = s.done[b];
                if (producer) {
                    if (tid == 0) {
                        const double last = s.tac[b ^ 1][kRowChunk - 1];  // (unused before the second chunk)
                        if (!done) tc_produce(it, s, b ^ 1, dt);  // the next chunk meanwhile
                        prev_tac = last;
                    }
                } else {
                    const int lane = tid - 64;
                    const int G = (cnt + kTcCheckers - 1) / kTcCheckers;
                    const int j0 = lane * G;
                    const int j1 = min(j0 + G, cnt);
                    const bool has = j0 < cnt;
                    double l[3] = {0.0, 0.0, 0.0};  // the lane's last sample
                    if (has) pos(j1 - 1, l);
                    // (whole wave: no lane has left the loop; a lane without samples hands up
                    // zeros, which only a lane without samples receives)
                    double q[3] = {__shfl_up(l[0], 1), __shfl_up(l[1], 1), __shfl_up(l[2], 1)};
                    if (lane == 0) {
                        q[0] = cx;
                        q[1] = cy;
                        q[2] = cz;
                    }
                    cx = __shfl(l[0], kTcCheckers - 1);  // (a full chunk: sample kRowChunk - 1; else unused)
                    cy = __shfl(l[1], kTcCheckers - 1);
                    cz = __shfl(l[2], kTcCheckers - 1);
                    if (has) {
                        for (int j = j0; j < j1; ++j) {
                            double e[3] = {l[0], l[1], l[2]};
                            if (j < j1 - 1) pos(j, e);
                            if ((base | j) != 0 && !ray_valid(a, w, q, e, cp)) {  // (row 0 ends no chord)
                                atomicMin(&s.first[b], j);  // (a lane's chords ascend: its first failure is its lowest)
                                break;
                            }
                            q[0] = e[0];
                            q[1] = e[1];
                            q[2] = e[2];
                        }
                    }
                }
                __syncthreads();
                const int f = s.first[b];
                if (f != INT_MAX) {
                    res = base + f - 1;  // the chord's start row
                    rtime = (f > 0 ? s.tac[b][f - 1] : prev_tac) + 0.0;  // epp_sample_batch's time column with t0 == NULL
                    break;
                }
                if (done) break;
                base += cnt;
                b ^= 1;
            }
        }
        if (tid == 0) {
            first_invalid[t] = res;
            if (first_time) first_time[t] = rtime;
        }
    }
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_traj_check_batch(const epp_world* world, const double* seg_times, const double* coeffs,
                                const int32_t* wp_offsets, int32_t n_tracks, double dt, double min_distance,
                                int64_t* first_invalid, double* first_time, void* stream) {
    if (!world || n_tracks < 0 || !(dt > 0) || !std::isfinite(dt) ||
        (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !first_invalid))) {
        set_error("epp_traj_check_batch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    IndexLease ix;  // (a stale index is rebuilt here, as by epp_check_states_mindist)
    if (const epp_status st = ensure_index(world, &ix)) return st;
    const WorldView& v = ix.view;
    // EPP_TRAJCHECK_STAGE=0: the front read through L2 whatever its size (A/B and test knob)
    const bool stage = v.front_bytes <= kTcFrontLds && env_int("EPP_TRAJCHECK_STAGE", 1) != 0;
    const uint32_t shm = kTcSharedBytes + (stage ? v.front_bytes : 0u);
    // persistent grid: as many workgroups as stay resident: 8 per CU by registers (97 VGPRs: 4 waves
    // per SIMD, 16 per CU, 2 per workgroup), fewer by LDS (7 with a small staged front)
    const int per_cu = std::max(1, std::min<int>(8, (int)((160u * 1024u) / shm)));
    const int grid = (int)std::min<int64_t>(n_tracks, (int64_t)cu_count() * per_cu);
    if (stage)
        hipLaunchKernelGGL((k_traj_check<true>), dim3(grid), dim3(kTcBlock), shm, (hipStream_t)stream, v, seg_times,
                           coeffs, wp_offsets, n_tracks, dt, min_distance, first_invalid, first_time, v.front_bytes);
    else
        hipLaunchKernelGGL((k_traj_check<false>), dim3(grid), dim3(kTcBlock), shm, (hipStream_t)stream, v, seg_times,
                           coeffs, wp_offsets, n_tracks, dt, min_distance, first_invalid, first_time, 0u);
    return launch_error("epp_traj_check_batch");
}

epp_status epp_traj_sweep_batch(const epp_world* world, const double* seg_times, const double* coeffs,
                                const int32_t* wp_offsets, int32_t n_tracks, double dt, int32_t can_pass_gate,
                                int64_t* first_invalid, double* first_time, void* stream) {
    if (!world || n_tracks < 0 || !(dt > 0) || !std::isfinite(dt) || (can_pass_gate != 0 && can_pass_gate != 1) ||
        (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !first_invalid))) {
        set_error("epp_traj_sweep_batch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    IndexLease ix;  // (a stale index is rebuilt here, as by epp_check_motions)
    if (const epp_status st = ensure_index(world, &ix)) return st;
    const WorldView& v = ix.view;
    // What the ray walk reads short of the SoA table (cell starts, cell lists, meta words) in
    // LDS when it fits, else the front alone, else nothing.  EPP_TRAJSWEEP_STAGE = 0 | 1 caps
    // the level (A/B and test knob): 0 reads the whole world through L2.
    const int cap = env_int("EPP_TRAJSWEEP_STAGE", 2);
    int level = 0;
    uint32_t bytes = 0;
    if (cap >= 2 && v.off_soa % 16 == 0 && v.off_soa <= kTsWorldLds) {
        level = 2;
        bytes = v.off_soa;
    } else if (cap >= 1 && v.front_bytes <= kTsWorldLds) {
        level = 1;
        bytes = v.front_bytes;
    }
    const uint32_t shm = kTcSharedBytes + bytes;
    // persistent grid: the workgroups that stay resident (2 waves each; 8 per CU, fewer by LDS)
    const int per_cu = std::max(1, std::min<int>(8, (int)((160u * 1024u) / shm)));
    const int grid = (int)std::min<int64_t>(n_tracks, (int64_t)cu_count() * per_cu);
#define EPP_LAUNCH_TS(LEVEL)                                                                                       \
    hipLaunchKernelGGL((k_traj_sweep<LEVEL>), dim3(grid), dim3(kTcBlock), shm, (hipStream_t)stream, v, seg_times, \
                       coeffs, wp_offsets, n_tracks, dt, can_pass_gate, first_invalid, first_time, bytes)
    if (level == 2)
        EPP_LAUNCH_TS(2);
    else if (level == 1)
        EPP_LAUNCH_TS(1);
    else
        EPP_LAUNCH_TS(0);
#undef EPP_LAUNCH_TS
    return launch_error("epp_traj_sweep_batch");
}

}  // extern "C"
