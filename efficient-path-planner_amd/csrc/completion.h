// completion.h — the completion slots of the synchronous latency paths, both halves (the
// small state / ray checks of small.hip, the refit kernels of minsnap_refit.hip, k_pb_emit of
// plan_batch.hip and their hosts).  A kernel's workgroups write their results into pinned host
// memory and then each publishes the call's sequence number in its own pinned slot
// (publish_done); the host polls the slots (wait_done) instead of synchronising the stream.
// Sequence numbers come from next_seq (never 0) and the slots are zeroed when their pinned
// block is allocated (PinnedBuf::grow(bytes, true)), so a fresh slot never reads as done.
#pragma once
#include <immintrin.h>

#include <chrono>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace epp {

#ifdef __HIPCC__
// Before lane 0 of a workgroup publishes its completion with a system-scope release store:
// every wave waits until its own stores are acknowledged by the memory system
// (s_waitcnt vmcnt(0) lgkmcnt(0)), and the barrier orders them before that store, whose
// release (an L2 write-back of the XCD, then the store) covers them.  The wait is inline
// assembly with a "memory" clobber (as wave_sync_lds, minsnap_solve.h): the compiler
// takes the s_waitcnt builtin to touch no memory and may move stores across it; the clobber
// keeps every earlier store before the wait.  One system-scope release per workgroup
// instead of a __threadfence_system() per wave: k_motions_small at 1,024 edges (64
// workgroups) 11.3 -> 7.5 us, one edge 5.4 -> 4.7 us (scripts/gpu_small_rays.sh; measured
// with the builtin form of the wait, the same instruction).
__device__ __forceinline__ void wg_stores_settled() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// The workgroup's results (every thread's earlier stores, in host memory) are made visible
// system-wide, then lane 0 publishes `seq` in the workgroup's own slot.  A null slot (an
// asynchronous launch: nobody polls) is a no-op.  Block-uniform arguments.
__device__ __forceinline__ void publish_done(uint32_t* slot, uint32_t seq) {
    if (!slot) return;
    wg_stores_settled();
    if (threadIdx.x == 0) __hip_atomic_store(slot, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif  // __HIPCC__

// The next call's sequence number of a per-thread counter: never 0, which fresh slots hold.
inline uint32_t next_seq(uint32_t& counter) { return ++counter ? counter : ++counter; }

struct WaitResult {
    enum Kind { kDone, kHipError, kNoSlots, kDeadline } kind;  // kNoSlots: the stream finished without its slots
    hipError_t err;                                            // (kHipError)
};

// Polls slots[0, n) until each holds `seq` (acquire: the workgroups' results are visible).
// The stream is queried every ~1k polls, so a launch that failed or finished without
// publishing ends the wait, as does `deadline_s` seconds of a stream still running (0: no
// deadline).  The callers turn the result into their own error convention.
inline WaitResult wait_done(const uint32_t* slots, int n, uint32_t seq, hipStream_t stream, double deadline_s) {
    auto all_done = [&] {
        int b = 0;
        while (b < n && __atomic_load_n(slots + b, __ATOMIC_ACQUIRE) == seq) ++b;
        return b == n;
    };
    std::chrono::steady_clock::time_point t0;
    if (deadline_s > 0) t0 = std::chrono::steady_clock::now();
    for (uint64_t spin = 0;; ++spin) {
        if (all_done()) return {WaitResult::kDone, hipSuccess};
        if ((spin & 1023) == 1023) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipErrorNotReady) {
                if (deadline_s > 0 &&
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > deadline_s)
                    return {WaitResult::kDeadline, q};
                continue;
            }
            if (q != hipSuccess) return {WaitResult::kHipError, q};
            if (all_done()) return {WaitResult::kDone, hipSuccess};
            return {WaitResult::kNoSlots, hipSuccess};
        }
        _mm_pause();
    }
}

}  // namespace epp
