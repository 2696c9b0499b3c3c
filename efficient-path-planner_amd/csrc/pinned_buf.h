// pinned_buf.h — a grow-on-demand pinned (page-locked) host buffer.  The growth policy (exact,
// x1.5, a floor) stays with the caller, who passes the final size; so does whatever must
// happen before the old block is freed (a stream synchronisation) or after the new one
// exists (a warm-up DMA).
#pragma once
#include <cstddef>
#include <cstring>
#include <utility>

#include <hip/hip_runtime_api.h>

namespace epp {

struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;

    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { free(); }

    // At least `bytes`: nothing when they fit, else the block is freed and a new one of
    // exactly `bytes` allocated (its contents are not kept; `zero` fills the new block --
    // completion slots must not start with a stale sequence number, completion.h).
    hipError_t grow(size_t bytes, bool zero = false) {
        if (bytes <= cap) return hipSuccess;
        free();
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = bytes;
        if (zero) std::memset(p, 0, bytes);
        return hipSuccess;
    }
    void free() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

}  // namespace epp
