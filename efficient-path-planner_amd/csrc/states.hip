// states.hip — the entry points of the batched state validity checks and the choice of
// kernel; the kernels and their launchers are in small.hip and states_*.hip
// (states_kernels.h).
#include "states_kernels.h"

using namespace epp;

namespace {

// Test hook (not for production use): EPP_STATES_KERNEL = v4 | generic skips the faster
// kernels, so every path can be checked against the oracle.
enum class StatesKernel { V5, V4, Generic };
StatesKernel forced_kernel() {
    const char* v = std::getenv("EPP_STATES_KERNEL");
    if (!v || !*v) return StatesKernel::V5;
    const std::string k(v);
    return k == "generic" ? StatesKernel::Generic : k == "v4" ? StatesKernel::V4 : StatesKernel::V5;
}

// Kernel choice on an indexed world, first fit: k_states_v5 when its staged part fits and the
// buffers are aligned, else k_states_v4 (aligned buffers), else k_states.
epp_status launch_states(const WorldView& w, const WorldView* dw, bool mindist, const double* xyz, int64_t n,
                         int32_t can_pass, double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid,
                         hipStream_t st, const char* what) {
    const StatesKernel want = forced_kernel();
    if (want == StatesKernel::V5 && states_v5_fits(w, mindist, xyz, n, valid))
        return launch_states_v5(w, mindist, xyz, n, can_pass, md, valid, compact_idx, n_valid, st, what);
    if (want != StatesKernel::Generic && states_v4_fits(xyz, n, valid))
        return launch_states_v4(w, dw, mindist, xyz, n, can_pass, md, valid, compact_idx, n_valid, st, what);
    return launch_states_generic(w, mindist, xyz, n, can_pass, md, valid, compact_idx, n_valid, st, what);
}

// Both entries: small batches (<= kSmallStates states, <= kSmallMaxObbs OBBs) take the
// brute-force k_states_small (small.hip; no index needed), the others launch_states.
// `what` names the entry in error texts.
epp_status check_states(const epp_world* world, const double* xyz, int64_t n, bool mindist, int32_t can_pass,
                        double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid, void* stream,
                        const char* what) {
    if (!world || n < 0 || (n > 0 && (!xyz || !valid)) || (compact_idx && !n_valid)) {
        set_error(std::string(what) + ": invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    hipStream_t st = (hipStream_t)stream;
    SmallWorld sw = small_world(world);
    if (small_states(sw, n)) {
        if (const epp_status e = launch_states_small(sw, mindist, xyz, n, can_pass, md, valid, compact_idx, n_valid, st))
            return e;
        return note_record_reader(world, sw, st);
    }
    sw.lease = {};  // (a stale index is rebuilt below)
    IndexLease ix;
    if (const epp_status e = ensure_index(world, &ix)) return e;
    return launch_states(ix.view, ix.dview, mindist, xyz, n, can_pass, md, valid, compact_idx, n_valid, st, what);
}

}  // namespace

extern "C" {

epp_status epp_check_states(const epp_world* world, const double* xyz, int64_t n, int32_t can_pass_gate,
                            uint8_t* valid, int32_t* compact_idx, int64_t* n_valid, void* stream) {
    return check_states(world, xyz, n, false, can_pass_gate, 0.0, valid, compact_idx, n_valid, stream,
                        "epp_check_states");
}

epp_status epp_check_states_mindist(const epp_world* world, const double* xyz, int64_t n, double min_distance,
                                    uint8_t* valid, void* stream) {
    return check_states(world, xyz, n, true, 0, min_distance, valid, nullptr, nullptr, stream,
                        "epp_check_states_mindist");
}

}  // extern "C"
