// stream_bufs.h — per-host-thread state of the single-track host paths (the refit,
// minsnap_refit.hip; the scaled fits, host_generate.cpp): a stream bound to the thread's
// current device, two pinned host buffers the kernels read / write directly (sized exactly)
// and a device scratch; all released and recreated when the thread's device changes.
#pragma once
#include <string>

#include <hip/hip_runtime_api.h>

#include "epp_internal.h"
#include "pinned_buf.h"

namespace epp {
namespace {

struct StreamBufs {
    hipStream_t s = nullptr;
    int dev = -1;
    PinnedBuf h_in, h_out;
    double* d_scr = nullptr;
    size_t scr_cap = 0;
    void release() {
        if (s) (void)hipStreamSynchronize(s);
        h_in.free();
        h_out.free();
        if (d_scr) (void)hipFree(d_scr);
        if (s) (void)hipStreamDestroy(s);
        d_scr = nullptr;
        s = nullptr;
        scr_cap = 0;
    }
    ~StreamBufs() { release(); }
    hipError_t bind() {
        int d = 0;
        (void)hipGetDevice(&d);
        if (d != dev) release();  // bound to another device: start over
        dev = d;
        if (s) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) s = nullptr;
        return e;
    }
    // (after bind) at least these sizes; a new h_out block starts zeroed when zero_out
    hipError_t ensure(size_t in_b, size_t out_b, size_t scr_b, bool zero_out = false) {
        if (in_b > h_in.cap || out_b > h_out.cap || scr_b > scr_cap)
            (void)hipStreamSynchronize(s);  // (the previous call's kernel has ended)
        hipError_t e = h_in.grow(in_b);
        if (e == hipSuccess) e = h_out.grow(out_b, zero_out);
        if (e == hipSuccess && scr_b > scr_cap) {
            if (d_scr) (void)hipFree(d_scr);
            d_scr = nullptr;
            scr_cap = 0;
            e = hipMalloc(reinterpret_cast<void**>(&d_scr), scr_b);
            if (e == hipSuccess) scr_cap = scr_b;
        }
        return e;
    }
};
epp_status buffers_error(hipError_t e) {
    set_error(std::string("generateTrajectory: buffers: ") + hipGetErrorString(e));
    return EPP_ERR_HIP;
}

}  // namespace
}  // namespace epp
