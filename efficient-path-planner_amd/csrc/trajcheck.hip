// trajcheck.hip — first collision of fitted trajectories, straight from their coefficients
// (gfx950): of their rows (k_traj_check) and of the chords between the rows (k_traj_sweep);
// and the clearance of their rows (k_traj_clearance, below: the closest approach to a
// collision OBB, where and against which), on the same walk; and the first hit of the first
// failing chord (k_traj_first_hit, below: how far into the chord and against which OBB); and
// the clearance of the chords (k_traj_chord_clearance, below: the closest approach of the
// straight chords between the rows, edge_clearance.h).
//
//   PathPlanner::checkTrajectoryValidity  src/PathPlanner.cpp:267-280, per track, over the rows
//   Trajectory::evaluateRange(0, max_time, dt)  src/trajectory.cpp:81-141 would produce, with
//   World::checkPointValidity(p, minDistance)   src/World.cpp:106-128
//
// One launch, no row written: the answer per track is the index (and time) of the first row
// whose position fails, exactly what epp_sample_batch followed by epp_check_states_mindist
// gives.  The pieces are the sampler's own (traj_sample.h: the time recurrence, its stepping
// loop and the fused Horner) and the state checks' own (collision_common.h: classify +
// pair_hit<true>), so the sample times, positions and booleans are the same bits.
//
// Shape: the walk of traj_walk.h (tc_walk: persistent workgroups of 2 waves, thread 0 runs the
// time recurrence a chunk ahead of the checking wave), one check body per kernel below.  The
// world's front (occupancy masks, cell starts) is staged in LDS once per workgroup when it is
// small; the cell lists and the OBB table are read through L1 / L2 (consecutive samples of a
// track fall into the same few cells).
#include <climits>
#include <cmath>

#include "clearance.h"
#include "collision_common.h"
#include "edge_clearance.h"
#include "first_hit.h"
#include "traj_sample.h"
#include "traj_walk.h"

namespace epp {
namespace {

// The walker's constants live in traj_walk.h: kTcSegLds = 40; (tests/clearance_inputs.py reads
// the number from this line, so it is held to the header's)
static_assert(kTcSegLds == 40, "update the comment above: the tests read kTcSegLds from it");

// The world is staged in LDS up to this size (the grid has ~2 cells per OBB, 12 B each: the
// front of worlds up to ~1000 OBBs); a larger one is read through L2.
constexpr uint32_t kTcWorldLds = 24 * 1024;

// The dynamic LDS array (Guideline 17) is [TcShared | the staged part of the world].  LEVEL: 0
// nothing staged, 1 the front (occupancy masks, cell starts), 2 the blob up to the SoA table
// (front, cell lists, meta words).
template <int LEVEL>
__device__ __forceinline__ Acc tc_stage(const WorldView& w, unsigned char* lds, uint32_t bytes) {
    const unsigned char* staged = LEVEL ? stage_world(w, lds + kTcSharedBytes, bytes) : w.blob;
    Acc a = make_acc(staged, w.blob, w);
    if (LEVEL == 2) {
        a.meta = reinterpret_cast<const uint32_t*>(staged + w.off_meta);
        a.co = reinterpret_cast<const uint16_t*>(staged + w.off_cell_obb);
    }
    return a;
}

// How the two first-failure checks end a track: thread 0 writes the walk's answer.
struct TcFirst {
    __device__ __forceinline__ void posted(const TcShared&, int, int, const double* __restrict__, int) {}
    __device__ __forceinline__ void end(int t, int tid, bool, int64_t res, double rtime,
                                        int64_t* __restrict__ first_invalid, double* __restrict__ first_time) {
        if (tid == 0) {
            first_invalid[t] = res;
            if (first_time) first_time[t] = rtime;
        }
    }
};

// The rows: World::checkPointValidity(p_j, minDistance).  A lane takes samples lane, + 64, ...
struct TcPoints : TcFirst {
    const Acc& a;
    const WorldView& w;
    double md;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void keep(const TcShared&, int) {}
    __device__ __forceinline__ void check(TcShared& s, int b, int cnt, int64_t, int lane,
                                          const double* __restrict__ coeffs, int seg0) {
        for (int j = lane; j < cnt; j += kTcCheckers) {
            double p[3];
            tc_pos(s, b, j, coeffs, seg0, p);
            if (!state_valid_scalar<true>(a, w, p[0], p[1], p[2], false, md)) {
                atomicMin(&s.first[b], j);  // (a lane's samples ascend: its first failure is its lowest)
                break;
            }
        }
    }
    __device__ __forceinline__ int row(int f) const { return f; }
    __device__ __forceinline__ double time(const TcShared& s, int b, int f) const { return s.tac[b][f]; }
};

// The chords between consecutive rows:
//   World::checkRayValid(p_j, p_j+1, canPassGate)  src/World.cpp:130-162; the answer per track
//   is the lowest j whose chord fails: epp_sample_batch + epp_check_motions (mode 0) on
//   consecutive rows.
// A checking lane takes G = ceil(cnt / 64) consecutive samples of the chunk (8 of a full one)
// and tests the chords that END at them, so every chord has one owner: the chord into a lane's
// first sample starts at the last sample of the lane before it, which that lane evaluates
// first and hands up (one ds_bpermute shift per coordinate); lane 0 takes the previous chunk's
// last position, carried in a register of wave 1 (lane 63's, broadcast).  Every position is
// evaluated once; the track's first row ends no chord.  The ray test is ray_valid
// (collision_common.h), the generic motion kernel's scalar walk: it reads cell starts, cell
// lists, meta words and the SoA table; everything before the table is staged in LDS when it
// fits (kTcWorldLds), else only the front, else nothing.
// LDS result word of a half: the lowest failing chord's END sample in the half (0: the chord
// from the previous chunk); its time is the START row's, which for 0 lies in the half the
// producer is overwriting: thread 0 keeps it (prev_tac) before it produces.
struct TcChords : TcFirst {
    const Acc& a;
    const WorldView& w;
    bool cp;
    double cx, cy, cz;  // wave 1: the previous chunk's last position
    double prev_tac;    // thread 0: the previous chunk's last time
    __device__ __forceinline__ void begin() { cx = cy = cz = prev_tac = 0.0; }
    __device__ __forceinline__ void keep(const TcShared& s, int b) {
        prev_tac = s.tac[b ^ 1][kRowChunk - 1];  // (unused before the second chunk)
    }
    __device__ __forceinline__ void check(TcShared& s, int b, int cnt, int64_t base, int lane,
                                          const double* __restrict__ coeffs, int seg0) {
        const int G = (cnt + kTcCheckers - 1) / kTcCheckers;
        const int j0 = lane * G;
        const int j1 = min(j0 + G, cnt);
        const bool has = j0 < cnt;
        double l[3] = {0.0, 0.0, 0.0};  // the lane's last sample
        if (has) tc_pos(s, b, j1 - 1, coeffs, seg0, l);
        // (whole wave: no lane has left the loop; a lane without samples hands up zeros,
        // which only a lane without samples receives)
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
                if (j < j1 - 1) tc_pos(s, b, j, coeffs, seg0, e);
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
    __device__ __forceinline__ int row(int f) const { return f - 1; }  // the chord's start row
    __device__ __forceinline__ double time(const TcShared& s, int b, int f) const {
        return f > 0 ? s.tac[b][f - 1] : prev_tac;
    }
};

// The first hit of the first failing chord (first_hit.h): TcChords finds the chord -- its own
// check, row and time, so the chord is epp_traj_sweep_batch's by construction -- and, once per
// track and only after a chord was posted, the checking wave answers where the chord row j ->
// row j + 1 is first blocked and by which OBB: every lane evaluates the two row positions
// (tc_pos: the bits the detection tested), lanes stride over all records of the world through
// L2 keeping a strict < minimum (a lane's indices ascend), and the wave min-reduces
// lexicographically on (t, index).  The chord's start row for a posted sample 0 is the
// previous chunk's last position, which check() is about to overwrite: it is kept (ox, oy, oz),
// and so is that row's time (otac: TcChords' prev_tac is thread 0's alone).
// time = t_j + t_hit * (t_j+1 - t_j) on the time columns epp_sample_batch writes with
// t0 == NULL.  A track without a failing chord keeps +inf, -1.0, -1.
struct TcHitOut {
    int can_pass;
    double* t_hit;
    double* time;
    int32_t* obb;
};
struct TcFirstHit : TcChords {
    TcHitOut out;
    double ox, oy, oz;  // wave 1: the last position of the chunk before the one being checked
    double otac, ctac;  // wave 1: that row's time; the same for the chunk being checked
    double ht, htime;   // wave 1: the track's answer
    int hobb;
    __device__ __forceinline__ void reset() {
        ht = HUGE_VAL;
        htime = -1.0;
        hobb = -1;
    }
    __device__ __forceinline__ void check(TcShared& s, int b, int cnt, int64_t base, int lane,
                                          const double* __restrict__ coeffs, int seg0) {
        ox = cx;
        oy = cy;
        oz = cz;
        otac = ctac;
        ctac = s.tac[b][kRowChunk - 1];  // (a full chunk's last row; else no chunk follows)
        TcChords::check(s, b, cnt, base, lane, coeffs, seg0);
    }
    __device__ __forceinline__ void posted(const TcShared& s, int b, int f, const double* __restrict__ coeffs,
                                           int seg0) {
        if (threadIdx.x < 64) return;  // (wave-uniform: the checking wave)
        const int lane = threadIdx.x - 64;
        double q[3] = {ox, oy, oz}, e[3];
        if (f > 0) tc_pos(s, b, f - 1, coeffs, seg0, q);
        tc_pos(s, b, f, coeffs, seg0, e);
        HitEdge g;
        g.set(q[0], q[1], q[2], e[0], e[1], e[2]);
        const double* recs = reinterpret_cast<const double*>(w.blob + w.off_aos);
        hit_min(recs, lane, w.n_obb, kTcCheckers, 0, g, w.r_gate, w.r_obst, cp, ht, hobb);
        for (int m = 32; m > 0; m >>= 1) {
            const double ot = __shfl_xor(ht, m);
            const int oo = __shfl_xor(hobb, m);
            const bool take = ot < ht || (ot == ht && oo < hobb);
            ht = take ? ot : ht;
            hobb = take ? oo : hobb;
        }
        // the two rows' time columns as epp_sample_batch writes them with t0 == NULL
        const double t0 = (f > 0 ? s.tac[b][f - 1] : otac) + 0.0, t1 = s.tac[b][f] + 0.0;
        htime = t0 + ht * (t1 - t0);
    }
    __device__ __forceinline__ void end(int t, int tid, bool walked, int64_t res, double rtime,
                                        int64_t* __restrict__ chord, double* __restrict__ first_time) {
        TcFirst::end(t, tid, walked, res, rtime, chord, first_time);
        if (tid == 64) {
            out.t_hit[t] = ht;
            if (out.time) out.time[t] = htime;
            if (out.obb) out.obb[t] = hobb;
        }
        reset();
    }
};

// The clearance of the rows: the minimum over a track's rows of the squared distance to the
// nearest collision OBB (clearance.h), where it is attained and against which OBB.  Nothing is
// ever posted to first[], so the walk visits every chunk of every track.  A checking lane
// takes samples lane, + 64, ... and keeps its best (d2, row, time, OBB) in registers across
// the chunks, updating on strict <: its rows ascend, so the earliest row wins within a lane,
// and within a row the lowest OBB index (clear_min_*).  At the track's end wave 1 reduces
// lexicographically by (d2, row).  A row with a non-finite position has a NaN or +inf d2 and
// never updates.  The first n_lds entries come from the LDS tile staged behind TcShared, the
// rest of a larger world from its records through L2.
struct TcClearOut {
    double* clearance;
    int32_t* nearest;
};
struct TcClear {
    const double* tile;   // LDS: entries [0, n_lds)
    const double* recs;   // the world's records
    int n_lds, n_obb;
    TcClearOut out;
    double bd2, btime;    // wave 1: the lane's best so far
    int64_t brow;
    int bobb;
    __device__ __forceinline__ void reset() {
        bd2 = HUGE_VAL;
        brow = -1;
        btime = -1.0;
        bobb = -1;
    }
    __device__ __forceinline__ void begin() { reset(); }
    __device__ __forceinline__ void keep(const TcShared&, int) {}
    __device__ __forceinline__ void check(TcShared& s, int b, int cnt, int64_t base, int lane,
                                          const double* __restrict__ coeffs, int seg0) {
        for (int j = lane; j < cnt; j += kTcCheckers) {
            double p[3];
            tc_pos(s, b, j, coeffs, seg0, p);
            double d2 = HUGE_VAL;
            int o = -1;
            clear_min_tile(tile, 0, n_lds, p[0], p[1], p[2], d2, o);
            clear_min_recs(recs, n_lds, n_obb, p[0], p[1], p[2], d2, o);
            const bool lt = d2 < bd2;
            bd2 = lt ? d2 : bd2;
            brow = lt ? base + j : brow;
            btime = lt ? s.tac[b][j] : btime;
            bobb = lt ? o : bobb;
        }
    }
    __device__ __forceinline__ int row(int f) const { return f; }                           // (never posted:
    __device__ __forceinline__ double time(const TcShared&, int, int) const { return 0.0; }  //  never asked)
    __device__ __forceinline__ void posted(const TcShared&, int, int, const double* __restrict__, int) {}
    __device__ __forceinline__ void end(int t, int tid, bool walked, int64_t, double, int64_t* __restrict__ row_out,
                                        double* __restrict__ time_out) {
        if (tid < 64) return;  // (wave-uniform: wave 1 holds the bests)
        if (!walked) reset();  // no segment, no row
        for (int m = 32; m > 0; m >>= 1) {
            const double od2 = __shfl_xor(bd2, m), otime = __shfl_xor(btime, m);
            const long long orow = __shfl_xor((long long)brow, m);
            const int oobb = __shfl_xor(bobb, m);
            const bool take = od2 < bd2 || (od2 == bd2 && orow < brow);
            bd2 = take ? od2 : bd2;
            brow = take ? orow : brow;
            btime = take ? otime : btime;
            bobb = take ? oobb : bobb;
        }
        if (tid == 64) {
            out.clearance[t] = sqrt(bd2);  // once, after the minimum
            if (row_out) row_out[t] = brow;
            if (time_out) time_out[t] = btime + 0.0;  // epp_sample_batch's time column with t0 == NULL
            if (out.nearest) out.nearest[t] = bobb;
        }
    }
};

// The clearance of the chords (edge_clearance.h): the minimum over a track's chords row j ->
// row j + 1 of the squared distance between the chord and the nearest collision OBB, which
// chord, how far into it, when, and against which OBB.  The chords are paired as TcChords pairs
// them -- a checking lane takes G = ceil(cnt / 64) consecutive samples and the chords that END
// at them, its first chord starting at the last sample of the lane before it (one shift per
// coordinate), lane 0's at the previous chunk's last position, carried in a register of wave 1
// -- and the best is kept as TcClear keeps it: nothing is ever posted, a lane's chords ascend
// within a chunk and from chunk to chunk, so a strict < leaves it its earliest chord, and at
// the track's end wave 1 reduces lexicographically by (d2, chord).  The chord from the
// previous chunk needs its start row's time, which lies in the half thread 0 is overwriting:
// wave 1 keeps each checked chunk's last time itself (ctac), so keep() has nothing to do.
// time = t_j + t * (t_j+1 - t_j) on the time columns epp_sample_batch writes with t0 == NULL.
// A chord with a non-finite end never updates (ClearEdge::finite).
struct TcChordClearOut {
    double* clearance;
    double* t;
    int32_t* nearest;
};
struct TcChordClear {
    const double* tile;   // LDS: entries [0, n_lds)
    const double* recs;   // the world's records
    int n_lds, n_obb;
    TcChordClearOut out;
    double cx, cy, cz;    // wave 1: the previous chunk's last position
    double ctac;          // wave 1: the previous chunk's last time
    double bd2, bt, btime;  // wave 1: the lane's best so far
    int64_t bchord;
    int bobb;
    __device__ __forceinline__ void reset() {
        bd2 = HUGE_VAL;
        bchord = -1;
        bt = btime = -1.0;
        bobb = -1;
    }
    __device__ __forceinline__ void begin() {
        reset();
        cx = cy = cz = ctac = 0.0;
    }
    __device__ __forceinline__ void keep(const TcShared&, int) {}
    __device__ __forceinline__ void check(TcShared& s, int b, int cnt, int64_t base, int lane,
                                          const double* __restrict__ coeffs, int seg0) {
        const double otac = ctac;        // the time of the row before this chunk's first
        ctac = s.tac[b][kRowChunk - 1];  // (a full chunk's last row; else no chunk follows)
        const int G = (cnt + kTcCheckers - 1) / kTcCheckers;
        const int j0 = lane * G;
        const int j1 = min(j0 + G, cnt);
        const bool has = j0 < cnt;
        double l[3] = {0.0, 0.0, 0.0};  // the lane's last sample
        if (has) tc_pos(s, b, j1 - 1, coeffs, seg0, l);
        // (whole wave, as TcChords::check: a lane without samples hands up zeros, which only a
        // lane without samples receives)
        double q[3] = {__shfl_up(l[0], 1), __shfl_up(l[1], 1), __shfl_up(l[2], 1)};
        if (lane == 0) {
            q[0] = cx;
            q[1] = cy;
            q[2] = cz;
        }
        cx = __shfl(l[0], kTcCheckers - 1);  // (a full chunk: sample kRowChunk - 1; else unused)
        cy = __shfl(l[1], kTcCheckers - 1);
        cz = __shfl(l[2], kTcCheckers - 1);
        if (!has) return;
        for (int j = j0; j < j1; ++j) {
            double e[3] = {l[0], l[1], l[2]};
            if (j < j1 - 1) tc_pos(s, b, j, coeffs, seg0, e);
            if ((base | j) != 0) {  // (row 0 ends no chord)
                ClearEdge g;
                g.set(q[0], q[1], q[2], e[0], e[1], e[2]);
                double d2 = HUGE_VAL, t = -1.0;
                int o = -1;
                edge_min_tile(tile, 0, n_lds, g, d2, t, o);
                edge_min_recs(recs, n_lds, n_obb, g, d2, t, o);
                // the two rows' time columns as epp_sample_batch writes them with t0 == NULL
                const double t0 = (j > 0 ? s.tac[b][j - 1] : otac) + 0.0, t1 = s.tac[b][j] + 0.0;
                const bool lt = d2 < bd2;
                bd2 = lt ? d2 : bd2;
                bchord = lt ? base + j - 1 : bchord;
                bt = lt ? t : bt;
                btime = lt ? t0 + t * (t1 - t0) : btime;
                bobb = lt ? o : bobb;
            }
            q[0] = e[0];
            q[1] = e[1];
            q[2] = e[2];
        }
    }
    __device__ __forceinline__ int row(int f) const { return f; }                           // (never posted:
    __device__ __forceinline__ double time(const TcShared&, int, int) const { return 0.0; }  //  never asked)
    __device__ __forceinline__ void posted(const TcShared&, int, int, const double* __restrict__, int) {}
    __device__ __forceinline__ void end(int t, int tid, bool walked, int64_t, double, int64_t* __restrict__ chord_out,
                                        double* __restrict__ time_out) {
        if (tid < 64) return;  // (wave-uniform: wave 1 holds the bests)
        if (!walked) reset();  // no segment, no chord
        for (int m = 32; m > 0; m >>= 1) {
            const double od2 = __shfl_xor(bd2, m), ot = __shfl_xor(bt, m), otime = __shfl_xor(btime, m);
            const long long ochord = __shfl_xor((long long)bchord, m);
            const int oobb = __shfl_xor(bobb, m);
            const bool take = od2 < bd2 || (od2 == bd2 && ochord < bchord);
            bd2 = take ? od2 : bd2;
            bchord = take ? ochord : bchord;
            bt = take ? ot : bt;
            btime = take ? otime : btime;
            bobb = take ? oobb : bobb;
        }
        if (tid == 64) {
            out.clearance[t] = sqrt(bd2);  // once, after the minimum
            if (chord_out) chord_out[t] = bchord;
            if (out.t) out.t[t] = bt;
            if (time_out) time_out[t] = btime;
            if (out.nearest) out.nearest[t] = bobb;
        }
    }
};

__global__ __launch_bounds__(kTcBlock) void k_traj_chord_clearance(WorldView w, const double* __restrict__ seg_times,
                                                                   const double* __restrict__ coeffs,
                                                                   const int32_t* __restrict__ wp_off, int n_tracks,
                                                                   double dt, TcChordClearOut out,
                                                                   int64_t* __restrict__ chord,
                                                                   double* __restrict__ time, uint32_t stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double* tile = reinterpret_cast<double*>(lds + kTcSharedBytes);
    const double* recs = reinterpret_cast<const double*>(w.blob + w.off_aos);
    const int n_lds = (int)(stage_bytes / (kClearDoubles * sizeof(double)));
    clear_stage(recs, 0, n_lds, tile, kTcBlock);
    __syncthreads();
    TcChordClear chk{tile, recs, n_lds, w.n_obb, out};
    chk.begin();
    tc_walk(*reinterpret_cast<TcShared*>(lds), seg_times, coeffs, wp_off, n_tracks, dt, chord, time, chk);
}

__global__ __launch_bounds__(kTcBlock) void k_traj_clearance(WorldView w, const double* __restrict__ seg_times,
                                                             const double* __restrict__ coeffs,
                                                             const int32_t* __restrict__ wp_off, int n_tracks,
                                                             double dt, TcClearOut out, int64_t* __restrict__ row,
                                                             double* __restrict__ time, uint32_t stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double* tile = reinterpret_cast<double*>(lds + kTcSharedBytes);
    const double* recs = reinterpret_cast<const double*>(w.blob + w.off_aos);
    const int n_lds = (int)(stage_bytes / (kClearDoubles * sizeof(double)));
    clear_stage(recs, 0, n_lds, tile, kTcBlock);
    __syncthreads();
    TcClear chk{tile, recs, n_lds, w.n_obb, out};
    chk.reset();
    tc_walk(*reinterpret_cast<TcShared*>(lds), seg_times, coeffs, wp_off, n_tracks, dt, row, time, chk);
}

template <bool STAGE>
__global__ __launch_bounds__(kTcBlock) void k_traj_check(WorldView w, const double* __restrict__ seg_times,
                                                         const double* __restrict__ coeffs,
                                                         const int32_t* __restrict__ wp_off, int n_tracks, double dt,
                                                         double md, int64_t* __restrict__ first_invalid,
                                                         double* __restrict__ first_time, uint32_t stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Acc a = tc_stage<STAGE ? 1 : 0>(w, lds, stage_bytes);
    tc_walk(*reinterpret_cast<TcShared*>(lds), seg_times, coeffs, wp_off, n_tracks, dt, first_invalid, first_time,
            TcPoints{{}, a, w, md});
}

template <int STAGE>
__global__ __launch_bounds__(kTcBlock) void k_traj_sweep(WorldView w, const double* __restrict__ seg_times,
                                                         const double* __restrict__ coeffs,
                                                         const int32_t* __restrict__ wp_off, int n_tracks, double dt,
                                                         int can_pass, int64_t* __restrict__ first_invalid,
                                                         double* __restrict__ first_time, uint32_t stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Acc a = tc_stage<STAGE>(w, lds, stage_bytes);
    tc_walk(*reinterpret_cast<TcShared*>(lds), seg_times, coeffs, wp_off, n_tracks, dt, first_invalid, first_time,
            TcChords{{}, a, w, can_pass != 0});
}

template <int STAGE>
__global__ __launch_bounds__(kTcBlock) void k_traj_first_hit(WorldView w, const double* __restrict__ seg_times,
                                                             const double* __restrict__ coeffs,
                                                             const int32_t* __restrict__ wp_off, int n_tracks,
                                                             double dt, TcHitOut out, int64_t* __restrict__ chord,
                                                             double* __restrict__ first_time, uint32_t stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Acc a = tc_stage<STAGE>(w, lds, stage_bytes);
    TcFirstHit chk{{{}, a, w, out.can_pass != 0}, out};
    chk.reset();
    tc_walk(*reinterpret_cast<TcShared*>(lds), seg_times, coeffs, wp_off, n_tracks, dt, chord, first_time, chk);
}

// What the ray walk of the chords reads short of the SoA table (cell starts, cell lists, meta
// words) in LDS when it fits, else the front alone, else nothing.  EPP_TRAJSWEEP_STAGE = 0 | 1
// caps the level (A/B and test knob): 0 reads the whole world through L2.
int sweep_stage(const WorldView& v, uint32_t& bytes) {
    const int cap = env_int("EPP_TRAJSWEEP_STAGE", 2);
    if (cap >= 2 && v.off_soa % 16 == 0 && v.off_soa <= kTcWorldLds) {
        bytes = v.off_soa;
        return 2;
    }
    if (cap >= 1 && v.front_bytes <= kTcWorldLds) {
        bytes = v.front_bytes;
        return 1;
    }
    return 0;
}

// The two clearance kernels: the first tile of entries in LDS; a larger world's remaining
// records are read through L2.  EPP_TRAJCLEAR_STAGE=0: every record through L2 (A/B and test
// knob)
int clear_tile_stage(const WorldView& v, uint32_t& bytes) {
    if (env_int("EPP_TRAJCLEAR_STAGE", 1) != 0)
        bytes = (uint32_t)std::min(v.n_obb, kClearTile) * (uint32_t)(kClearDoubles * sizeof(double));
    return 0;
}

// What both entry points do around their kernels.  P: the check's own parameter (kernel
// argument 7); ok: the entry point's own argument checks (its required output among them); kernels: its kernel per staging
// level; stage(view, bytes): the level for this world, and how many bytes it stages.
template <class P>
using TcKernel = void (*)(WorldView, const double*, const double*, const int32_t*, int, double, P, int64_t*, double*,
                          uint32_t);

template <class P, class Stage>
epp_status tc_launch(const char* fn, bool ok, const TcKernel<P>* kernels, Stage stage, const epp_world* world,
                     const double* seg_times, const double* coeffs, const int32_t* wp_offsets, int32_t n_tracks,
                     double dt, P param, int64_t* first_invalid, double* first_time, void* stream) {
    if (!ok || !world || n_tracks < 0 || !(dt > 0) || !std::isfinite(dt) ||
        (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets))) {
        set_error(std::string(fn) + ": invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    IndexLease ix;  // (a stale index is rebuilt here, as by epp_check_states_mindist / epp_check_motions)
    if (const epp_status st = ensure_index(world, &ix)) return st;
    const WorldView& v = ix.view;
    uint32_t bytes = 0;
    const int level = stage(v, bytes);
    const uint32_t shm = kTcSharedBytes + bytes;
    // persistent grid: as many workgroups as stay resident: 8 per CU by registers (at most 128
    // VGPRs: 4 waves per SIMD, 16 per CU, 2 per workgroup), fewer by LDS (7 with a small staged front)
    const int per_cu = std::max(1, std::min<int>(8, (int)((160u * 1024u) / shm)));
    const int grid = (int)std::min<int64_t>(n_tracks, (int64_t)cu_count() * per_cu);
    hipLaunchKernelGGL(kernels[level], dim3(grid), dim3(kTcBlock), shm, (hipStream_t)stream, v, seg_times, coeffs,
                       wp_offsets, n_tracks, dt, param, first_invalid, first_time, bytes);
    return launch_error(fn);
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_traj_check_batch(const epp_world* world, const double* seg_times, const double* coeffs,
                                const int32_t* wp_offsets, int32_t n_tracks, double dt, double min_distance,
                                int64_t* first_invalid, double* first_time, void* stream) {
    static constexpr TcKernel<double> kernels[] = {k_traj_check<false>, k_traj_check<true>};
    // The front in LDS when it fits.  EPP_TRAJCHECK_STAGE=0: read through L2 whatever its
    // size (A/B and test knob)
    const auto stage = [](const WorldView& v, uint32_t& bytes) {
        if (v.front_bytes > kTcWorldLds || env_int("EPP_TRAJCHECK_STAGE", 1) == 0) return 0;
        bytes = v.front_bytes;
        return 1;
    };
    return tc_launch("epp_traj_check_batch", n_tracks <= 0 || first_invalid, kernels, stage, world, seg_times, coeffs, wp_offsets, n_tracks, dt,
                     min_distance, first_invalid, first_time, stream);
}

epp_status epp_traj_sweep_batch(const epp_world* world, const double* seg_times, const double* coeffs,
                                const int32_t* wp_offsets, int32_t n_tracks, double dt, int32_t can_pass_gate,
                                int64_t* first_invalid, double* first_time, void* stream) {
    static constexpr TcKernel<int> kernels[] = {k_traj_sweep<0>, k_traj_sweep<1>, k_traj_sweep<2>};
    return tc_launch("epp_traj_sweep_batch", (can_pass_gate == 0 || can_pass_gate == 1) && (n_tracks <= 0 || first_invalid),
                     kernels, sweep_stage, world,
                     seg_times, coeffs, wp_offsets, n_tracks, dt, (int)can_pass_gate, first_invalid, first_time,
                     stream);
}

epp_status epp_traj_first_hit_batch(const epp_world* world, const double* seg_times, const double* coeffs,
                                    const int32_t* wp_offsets, int32_t n_tracks, double dt, int32_t can_pass_gate,
                                    int64_t* chord, double* t_hit, double* time, int32_t* obb, void* stream) {
    static constexpr TcKernel<TcHitOut> kernels[] = {k_traj_first_hit<0>, k_traj_first_hit<1>, k_traj_first_hit<2>};
    return tc_launch("epp_traj_first_hit_batch",
                     (can_pass_gate == 0 || can_pass_gate == 1) && (n_tracks <= 0 || (chord && t_hit)), kernels,
                     sweep_stage, world, seg_times, coeffs, wp_offsets, n_tracks, dt,
                     TcHitOut{(int)can_pass_gate, t_hit, time, obb}, chord, nullptr, stream);
}

epp_status epp_traj_clearance_batch(const epp_world* world, const double* seg_times, const double* coeffs,
                                    const int32_t* wp_offsets, int32_t n_tracks, double dt, double* clearance,
                                    int64_t* row, double* time, int32_t* nearest, void* stream) {
    static constexpr TcKernel<TcClearOut> kernels[] = {k_traj_clearance};
    return tc_launch("epp_traj_clearance_batch", n_tracks <= 0 || clearance, kernels, clear_tile_stage, world,
                     seg_times, coeffs, wp_offsets, n_tracks, dt, TcClearOut{clearance, nearest}, row, time, stream);
}

epp_status epp_traj_chord_clearance_batch(const epp_world* world, const double* seg_times, const double* coeffs,
                                          const int32_t* wp_offsets, int32_t n_tracks, double dt, double* clearance,
                                          int64_t* chord, double* t, double* time, int32_t* nearest, void* stream) {
    static constexpr TcKernel<TcChordClearOut> kernels[] = {k_traj_chord_clearance};
    return tc_launch("epp_traj_chord_clearance_batch", n_tracks <= 0 || clearance, kernels, clear_tile_stage, world,
                     seg_times, coeffs, wp_offsets, n_tracks, dt, TcChordClearOut{clearance, t, nearest}, chord, time,
                     stream);
}

}  // extern "C"
