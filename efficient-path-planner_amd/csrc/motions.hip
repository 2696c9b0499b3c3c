// motions.hip — the entry points of the batched motion (edge) validity checks and the choice
// of kernel; the kernels and their launchers are in small.hip and motions_*.hip
// (motions_kernels.h).
#include "collision_common.h"
#include "motions_kernels.h"

using namespace epp;

namespace {

// What the k-NN-table entries share: the refusals, the index, the tile launch (the only
// kernel that reads a table).  refuse_small: not for a batch the small path would take, nor
// with EPP_MOTIONS_KERNEL set (to anything).  `why` completes the EPP_ERR_UNSUPPORTED text.
epp_status check_knn_table(const char* what, const char* why, bool refuse_small, const epp_world* world,
                           const double* nodes, const int32_t* nbr, int32_t k, int64_t m, int32_t can_pass_gate,
                           int32_t mode, uint8_t* valid, void* stream, const MotionMask& mm) {
    auto unsupported = [&] {
        set_error(std::string(what) + why);
        return EPP_ERR_UNSUPPORTED;
    };
    if (refuse_small) {
        const SmallWorld sw = small_world(world);
        if (small_motions(sw, m) || std::getenv("EPP_MOTIONS_KERNEL")) return unsupported();
    }  // (sw's lease ends here: a stale index is rebuilt below)
    IndexLease ix;
    if (const epp_status st = ensure_index(world, &ix)) return st;
    if (!launch_motions_tile(ix.dview, ix.view, nodes, nullptr, nbr, k, m, can_pass_gate, mode, valid,
                             (hipStream_t)stream, mm))
        return unsupported();
    return launch_error(what);
}

// The planner's edge mask from an entry's arguments.
MotionMask edge_mask(int32_t* nbr_w, uint16_t* out16, int32_t target, int64_t* count) {
    MotionMask mm;
    mm.nbr_w = nbr_w;
    mm.out16 = out16;
    mm.target = target;
    mm.count = reinterpret_cast<unsigned long long*>(count);
    return mm;
}

}  // namespace

extern "C" {

// Kernel choice, first fit: small batches (<= kSmallMotions edges, <= kSmallMaxObbs OBBs)
// take the brute-force k_motions_small (no index needed); else the tile kernel; else the
// cell-list kernels; else k_motions.  Test hooks (not for production use):
// EPP_MOTIONS_KERNEL set to anything but "small" skips the small path, =generic forces
// k_motions, =v4 skips the tile kernel.
epp_status epp_check_motions(const epp_world* world, const double* s1, const double* s2, int64_t n,
                             int32_t can_pass_gate, int32_t mode, uint8_t* valid, void* stream) {
    if (!world || n < 0 || (n > 0 && (!s1 || !s2 || !valid)) || (mode != 0 && mode != 1)) {
        set_error("epp_check_motions: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    hipStream_t st = (hipStream_t)stream;
    SmallWorld sw = small_world(world);
    if (small_motions(sw, n)) {
        if (const epp_status e = launch_motions_small(sw, mode, s1, s2, n, can_pass_gate != 0 ? 1 : 0, valid, st))
            return e;
        return note_record_reader(world, sw, st);
    }
    sw.lease = {};  // (a stale index is rebuilt below)
    IndexLease ix;
    if (const epp_status e = ensure_index(world, &ix)) return e;
    const char* forced = std::getenv("EPP_MOTIONS_KERNEL");
    const bool generic = forced && std::string(forced) == "generic";
    const bool v4 = forced && std::string(forced) == "v4";
    bool launched = false;
    if (!generic && !v4)
        launched = launch_motions_tile(ix.dview, ix.view, s1, s2, nullptr, 1, n, can_pass_gate, mode, valid, st);
    if (!launched && !generic)
        launched = launch_motions_cells(ix.dview, ix.view, s1, s2, n, can_pass_gate, mode, valid, st);
    if (!launched) launch_motions_generic(ix.view, s1, s2, n, can_pass_gate, mode, valid, st);
    return launch_error("epp_check_motions");
}

epp_status epp_check_knn_motions(const epp_world* world, const double* nodes, const int32_t* nbr, int32_t n,
                                 int32_t k, int32_t can_pass_gate, int32_t mode, uint8_t* valid, void* stream) {
    if (!world || n < 0 || k <= 0 || (n > 0 && (!nodes || !nbr || !valid)) || (mode != 0 && mode != 1)) {
        set_error("epp_check_knn_motions: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    const int64_t m = (int64_t)n * k;
    if (m == 0) return EPP_OK;
    return check_knn_table("epp_check_knn_motions",
                           ": not for this batch / world (use epp_knn_edges + epp_check_motions)", true, world, nodes,
                           nbr, k, m, can_pass_gate, mode, valid, stream, MotionMask{});
}

}  // extern "C"

epp_status epp::check_knn_motions_masked(const epp_world* world, const double* nodes, int32_t* nbr, int32_t n,
                                         int32_t k, int32_t can_pass_gate, uint8_t* valid, uint16_t* out16,
                                         int32_t target, int64_t* count, void* stream) {
    if (!world || n < 0 || k <= 0 || (n > 0 && (!nodes || !nbr || !valid || !count))) {
        set_error("check_knn_motions_masked: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    const int64_t m = (int64_t)n * k;
    if (m == 0) return EPP_OK;
    return check_knn_table("check_knn_motions_masked", ": not for this batch / world", true, world, nodes, nbr, k, m,
                           can_pass_gate, 0, valid, stream, edge_mask(nbr, out16, target, count));
}

bool epp::knn_motions_rows_supported(const epp_world* world) {
    if (!world) return false;
    IndexLease ix;
    if (ensure_index(world, &ix) != EPP_OK) return false;
    return motions_tile_fits(ix.view);
}

epp_status epp::check_knn_motions_rows(const epp_world* world, const double* nodes, int32_t* rows32,
                                       const int32_t* ids32, const int64_t* rows_n, int32_t cap, int32_t k,
                                       int32_t can_pass_gate, uint8_t* valid, uint16_t* out16, int32_t target,
                                       int64_t* count, void* stream, const MotionMask* marks) {
    if (!world || cap < 0 || k <= 0 || (cap > 0 && (!nodes || !rows32 || !ids32 || !rows_n || !valid || (!count && !out16))) ||
        (marks && marks->mark && (!out16 || !marks->pkept || !marks->pgoal || marks->nprob < 1 || marks->nprob > 64))) {
        set_error("check_knn_motions_rows: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    const int64_t m = (int64_t)cap * k;
    if (m == 0) return EPP_OK;
    MotionMask mm = edge_mask(rows32, out16, target, count);
    mm.rowmap = ids32;
    mm.rows_n = reinterpret_cast<const unsigned long long*>(rows_n);
    if (marks) {
        mm.mark = marks->mark;
        mm.pkept = marks->pkept;
        mm.pgoal = marks->pgoal;
        mm.ns_log = marks->ns_log;
        mm.nprob = marks->nprob;
    }
    // (the planner's own rows: neither the small path nor EPP_MOTIONS_KERNEL applies)
    return check_knn_table("check_knn_motions_rows", ": not for this world", false, world, nodes, rows32, k, m,
                           can_pass_gate, 0, valid, stream, mm);
}
