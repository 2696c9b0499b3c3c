// traj_walk.h — the walk over fitted tracks that every k_traj_* kernel runs (trajcheck.hip:
// k_traj_check, k_traj_sweep, k_traj_first_hit, k_traj_clearance, k_traj_chord_clearance;
// gate_pass.hip: k_traj_gates;
// thrust_rates.hip: k_traj_thrust_rates):
// the LDS double buffer of the time recurrence (TcShared), its producer, the position of a
// sample (tc_pos) and tc_walk, whose check body is a template parameter.  One definition, so
// every kernel walks the same samples bit for bit.
//
// Shape (tc_walk): persistent workgroups of 2 waves, each taking tracks blockIdx.x,
// + gridDim.x, ...  The time recurrence is sequential: thread 0 runs it kRowChunk samples at a
// time into one half of a double buffer in LDS (time in segment, time, segment) while wave 1
// evaluates and checks the other half.  A failing lane posts its sample's index with an LDS
// min; after the chunk's barrier the lowest one, if any, is the track's answer and the
// workgroup moves on, so an early finding costs at most one chunk of look-ahead.  The launch
// is bound by the recurrence, so what counts is how many of them run at
// once: two waves per workgroup (one checking wave keeps up with the recurrence) let ~7
// workgroups share a CU; with four waves (three checking) 4 did and the launch took 1.5 times
// as long.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "traj_sample.h"

namespace epp {
namespace {

constexpr int kTcBlock = 128;
constexpr int kTcCheckers = kTcBlock - 64;  // lanes of wave 1
// Segment times staged in LDS (the tracks epp_minsnap_batch fits in LDS); a longer track's
// recurrence reads them through L2: one read per segment either way.
constexpr int kTcSegLds = 40;

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

// The next (up to) kRowChunk samples of the recurrence into half b.  Also clears the half's
// result word, so each half carries its own from production to the read after its check.
__device__ __forceinline__ void tc_produce(RangeIter& it, TcShared& s, int b, double dt) {
    int done = 0;
    s.cnt[b] = range_produce(it, dt, kRowChunk, s.seg[b], s.tin[b], s.tac[b], done);
    s.done[b] = done;
    s.first[b] = INT_MAX;
}

// The position of sample j of half b.
__device__ __forceinline__ void tc_pos(const TcShared& s, int b, int j, const double* __restrict__ coeffs, int seg0,
                                       double (&p)[3]) {
    const double* cs = coeffs + (size_t)(seg0 + s.seg[b][j]) * (3 * kPolyCoeffs);
    const double tin = s.tin[b][j];
    p[0] = poly_eval_pos(cs, tin);
    p[1] = poly_eval_pos(cs + kPolyCoeffs, tin);
    p[2] = poly_eval_pos(cs + 2 * kPolyCoeffs, tin);
}

// The walk over the tracks.  Check is what wave 1 does with a half and how a posted sample
// becomes the answer:
//   begin()                         a track starts (every thread)
//   keep(s, b)                      thread 0, before it overwrites half b ^ 1
//   check(s, b, cnt, base, lane, coeffs, seg0)   wave 1: atomicMin(&s.first[b], j) for a failing j
//   row(f), time(s, b, f)           the answer for posted sample f of half b, relative to base
//   posted(s, b, f, coeffs, seg0)   every thread, once per track with a posted sample, while
//                                   half b is still intact: what a check adds to that answer
//   end(t, tid, walked, res, rtime, first_invalid, first_time)   the track is over (every thread;
//                                   walked: it had a segment): write its outputs.  A check that
//                                   never posts walks every chunk and answers from its own state.
template <class Check>
__device__ __forceinline__ void tc_walk(TcShared& s, const double* __restrict__ seg_times,
                                        const double* __restrict__ coeffs, const int32_t* __restrict__ wp_off,
                                        int n_tracks, double dt, int64_t* __restrict__ first_invalid,
                                        double* __restrict__ first_time, Check chk) {
    const int tid = threadIdx.x;
    const bool producer = tid < 64;  // wave 0 (its lane 0 runs the recurrence)
    RangeIter it;                    // (thread 0's)
    for (int t = blockIdx.x; t < n_tracks; t += gridDim.x) {
        const int w0 = wp_off[t];
        const int M = wp_off[t + 1] - w0 - 1;
        int64_t res = -1;  // nothing fails (also: no segment, no row: the reference loop returns true)
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
            chk.begin();
            // One barrier per chunk.  Ordering of the LDS accesses around it, for half b checked
            // in this iteration and half b ^ 1 produced in it:
            //  - everything of half b (samples, cnt, done, first = INT_MAX) was written by thread 0
            //    before the previous barrier; this iteration only the checkers' atomicMin touches
            //    first[b], before the barrier, and every thread reads first[b] after it;
            //  - thread 0 writes half b ^ 1 (first[b ^ 1] included) before the barrier; its last
            //    readers read it before the previous barrier, or after it only first[b ^ 1],
            //    which then held INT_MAX (a smaller value ended the track) -- the value written --
            //    and what keep() takes, which thread 0 itself reads before it writes;
            //  - the next iteration's checkers post to first[b ^ 1], never to the word a slow
            //    wave may still be reading, so both waves take the same decision;
            //  - a track's end is followed by the next track's first barrier before any write.
            for (;;) {
                const int cnt = s.cnt[b], done = s.done[b];
                if (producer) {
                    if (tid == 0) {
                        chk.keep(s, b);
                        if (!done) tc_produce(it, s, b ^ 1, dt);  // the next chunk meanwhile
                    }
                } else {
                    chk.check(s, b, cnt, base, tid - 64, coeffs, seg0);
                }
                __syncthreads();
                const int f = s.first[b];
                if (f != INT_MAX) {
                    res = base + chk.row(f);
                    rtime = chk.time(s, b, f) + 0.0;  // epp_sample_batch's time column with t0 == NULL
                    chk.posted(s, b, f, coeffs, seg0);
                    break;
                }
                if (done) break;
                base += cnt;
                b ^= 1;
            }
        }
        chk.end(t, tid, M >= 1, res, rtime, first_invalid, first_time);
    }
}

}  // namespace
}  // namespace epp
