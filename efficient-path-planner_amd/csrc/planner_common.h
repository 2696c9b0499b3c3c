// planner_common.h — what the planner's device files (planner.hip, knn*.hip via knn_grid.h,
// plan_batch.hip) share: the uniform sampler, the decoupled look-back of the single-pass
// ordered scans, the ordered compaction's chunk shape, and the scan tag planner.hip
// hands out for all three.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "epp_internal.h"
#include "launch_helpers.h"  // cu_count, launch_error

namespace epp {

// (planner.hip)
uint32_t next_scan_tag();  // a launch tag for lb_publish / lb_exclusive: 24 bits, never 0

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Sample `index` of the counter-based uniform sampler over the box [lo, hi]: three
// splitmix64 draws (counters 3 index .. 3 index + 2), 53 bits each.  k_sample_uniform and
// k_pb_sample give the same doubles for the same (seed, index).
__device__ __forceinline__ void sample_uniform(uint64_t seed, uint64_t index, const double (&lo)[3],
                                               const double (&hi)[3], double* __restrict__ x) {
    const uint64_t c = index * 3ull;
    const double u0 = (double)(splitmix64(seed ^ c) >> 11) * 0x1.0p-53;
    const double u1 = (double)(splitmix64(seed ^ (c + 1)) >> 11) * 0x1.0p-53;
    const double u2 = (double)(splitmix64(seed ^ (c + 2)) >> 11) * 0x1.0p-53;
    x[0] = lo[0] + (hi[0] - lo[0]) * u0;
    x[1] = lo[1] + (hi[1] - lo[1]) * u1;
    x[2] = lo[2] + (hi[2] - lo[2]) * u2;
}

// ---- decoupled look-back (single-pass ordered scans) ---------------------------------
// A block publishes its chunk's total as soon as it has counted it ("aggregate"), then
// its inclusive prefix once it knows its exclusive one.  Its look-back reads the status
// words of the 64 blocks before it at once (one lane each), waits for every one of them to
// be published in this launch, and sums back to the nearest inclusive prefix -- no
// block waits on a chain of predecessors (they publish their aggregates without waiting).
// Status word: [63..40] launch tag (24 bits, never 0), [39] inclusive flag, [38..0] value.
// The status words are zeroed on the stream before every launch (a zero word carries no
// tag, so it reads as unpublished); the tag is a second guard, against a word published by
// an earlier launch on another stream.  Blocks only wait on lower-numbered blocks, which are
// dispatched first, so the wait always ends.
constexpr int kTagShift = 40;
constexpr unsigned long long kIncl = 1ull << 39, kValMask = kIncl - 1ull;
__device__ __forceinline__ void lb_publish(unsigned long long* st, int b, uint32_t tag, bool incl, long long v) {
    const unsigned long long w = ((unsigned long long)tag << kTagShift) | (incl ? kIncl : 0ull) | ((unsigned long long)v & kValMask);
    __hip_atomic_store(st + b, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Exclusive prefix of block b (called by one whole wavefront; every lane gets it).
__device__ __forceinline__ long long lb_exclusive(unsigned long long* st, int b, uint32_t tag) {
    const int lane = threadIdx.x & 63;
    long long acc = 0;
    for (int hi = b - 1; hi >= 0; hi -= 64) {  // window [hi - 63, hi], lane l reads block hi - l
        const int j = hi - lane;
        unsigned long long w = 0ull;
        if (j >= 0) {
            do w = __hip_atomic_load(st + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while ((uint32_t)(w >> kTagShift) != tag);
        }
        const unsigned long long pm = __ballot(j >= 0 && (w & kIncl));
        // the nearest inclusive prefix (lowest lane with one) ends the walk
        const int stop = pm ? __builtin_ctzll(pm) : 64;
        long long v = (lane <= stop && j >= 0) ? (long long)(w & kValMask) : 0ll;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        acc += v;
        if (pm) break;
    }
    return acc;
}

// The ordered compaction's chunk (planner.hip's compact_block; k_pb_compact and k_pb_number
// in plan_batch.hip): block b owns kCompactChunk consecutive entries, in kCompactRounds
// rounds of one entry per thread.
constexpr int kCompactThreads = 256;
constexpr int kCompactRounds = 4;
constexpr int kCompactChunk = kCompactThreads * kCompactRounds;

}  // namespace
}  // namespace epp
