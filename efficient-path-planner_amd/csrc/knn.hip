// knn.hip — the epp_knn* entry points (include/epp.h) of the exact k-NN: validate, take a
// workspace, build the grid, query, retry.  The kernels and their launchers are knn_build.hip,
// knn_walk.hip, knn_tile.hip and knn_retry.hip; knn_kernels.h has the overview.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>

#include "cached_ws.h"
#include "epp_internal.h"
#include "knn_kernels.h"

namespace epp {
namespace {

// Tables up to this size go to the all-pairs kernel: the grid pays off from a few thousand
// nodes; both give the same answer.
constexpr int kKnnBruteMax = 2048;

bool knn_args_ok(const char* name, const double* nodes, int n, int k, const int32_t* nbr, bool more_ok = true,
                 const char* more = "") {
    if (n < 0 || (n > 0 && (!nodes || !nbr)) || (k != 4 && k != 8 && k != 16 && k != 32) || !more_ok) {
        set_error(std::string(name) + ": invalid argument (k must be 4, 8, 16 or 32" + more + ")");
        return false;
    }
    return true;
}

bool knn_ws_ok(const char* name, const void* ws, uint64_t ws_bytes, const KnnLayout& L) {
    if (!ws || ws_bytes < L.bytes || (reinterpret_cast<uintptr_t>(ws) & 255)) {
        set_error(std::string(name) + ": workspace missing, unaligned or smaller than epp_knn_workspace_size(n)");
        return false;
    }
    return true;
}

// The grid pipeline on a workspace: build, then the query kernel for k.
epp_status knn_grid_launch(const double* nodes, int n, int k, double max_dist, int32_t* nbr, char* buf,
                           const KnnLayout& L, hipStream_t s, const double* box_lo = nullptr,
                           const double* box_hi = nullptr) {
    const KnnWs w = knn_ws_parts(buf, L);
    const double r2 = knn_r2max(max_dist);
    knn_build_launch(nodes, n, w, s, box_lo, box_hi);
    // EPP_KNN_TILE=0 selects the untiled grid walk (same answers; a test hook); the default is
    // k_knn_tile.  (A one-query-per-lane variant that keeps the exact
    // top-K in registers straight out of an LDS copy of the halo was tried: 425 us per
    // 63k-node table against k_knn_tile's 134 us -- the sorted insert then runs for nearly
    // every candidate of every lane.)
    const char* tile_env = std::getenv("EPP_KNN_TILE");
    const bool tiled = !(tile_env && *tile_env) || std::atoi(tile_env) != 0;
    if (tiled && (k == 4 || k == 8 || k == 16)) {
        const int cus = cu_count();
        knn_tile_launch(k, cus, nodes, r2, w, nbr, s);
        knn_retry_launch(k, cus, nodes, r2, w, nbr, s);
    } else {
        knn_walk_launch(k, n, r2, w, nbr, s);
    }
    return launch_error("epp_knn_grid");
}

CachedWs g_knn_ws[64];

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_knn_bruteforce(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr,
                              void* stream) {
    if (!knn_args_ok("epp_knn", nodes, n, k, nbr)) return EPP_ERR_INVALID_ARGUMENT;
    if (n == 0) return EPP_OK;
    knn_brute_launch(k, nodes, n, knn_r2max(max_dist), nbr, (hipStream_t)stream);
    return launch_error("epp_knn_bruteforce");
}

epp_status epp_knn(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* stream) {
    // (EPP_KNN_IMPL=1 / 2 forces all-pairs / grid: diagnostics)
    const char* f = std::getenv("EPP_KNN_IMPL");
    const int impl = f && *f ? std::atoi(f) : 0;
    const bool brute = impl == 1 || (impl == 0 && n <= kKnnBruteMax);
    return brute ? epp_knn_bruteforce(nodes, n, k, max_dist, nbr, stream)
                 : epp_knn_grid(nodes, n, k, max_dist, nbr, stream);
}

uint64_t epp_knn_workspace_size(int32_t n) { return n <= 0 ? 0 : (uint64_t)knn_layout(n).bytes; }

epp_status epp_knn_ws(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* ws,
                      uint64_t ws_bytes, void* stream) {
    if (n > kKnnBruteMax) return epp_knn_grid_ws(nodes, n, k, max_dist, nbr, ws, ws_bytes, stream);
    return epp_knn_bruteforce(nodes, n, k, max_dist, nbr, stream);
}

epp_status epp_knn_grid_ws_box(const double* nodes, int32_t n, int32_t k, double max_dist, const double lo[3],
                               const double hi[3], int32_t* nbr, void* ws, uint64_t ws_bytes, void* stream) {
    const bool box_ok = lo && hi && lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
    if (!knn_args_ok("epp_knn_grid_ws_box", nodes, n, k, nbr, box_ok, "; lo <= hi")) return EPP_ERR_INVALID_ARGUMENT;
    if (n == 0) return EPP_OK;
    const KnnLayout L = knn_layout(n);
    if (!knn_ws_ok("epp_knn_grid_ws_box", ws, ws_bytes, L)) return EPP_ERR_INVALID_ARGUMENT;
    return knn_grid_launch(nodes, n, k, max_dist, nbr, static_cast<char*>(ws), L, (hipStream_t)stream, lo, hi);
}

epp_status epp_knn_ws_box(const double* nodes, int32_t n, int32_t k, double max_dist, const double lo[3],
                          const double hi[3], int32_t* nbr, void* ws, uint64_t ws_bytes, void* stream) {
    if (n > kKnnBruteMax) return epp_knn_grid_ws_box(nodes, n, k, max_dist, lo, hi, nbr, ws, ws_bytes, stream);
    return epp_knn_bruteforce(nodes, n, k, max_dist, nbr, stream);
}

epp_status epp_knn_grid_ws(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* ws,
                           uint64_t ws_bytes, void* stream) {
    if (!knn_args_ok("epp_knn_grid", nodes, n, k, nbr)) return EPP_ERR_INVALID_ARGUMENT;
    if (n == 0) return EPP_OK;
    const KnnLayout L = knn_layout(n);
    if (!knn_ws_ok("epp_knn_grid", ws, ws_bytes, L)) return EPP_ERR_INVALID_ARGUMENT;
    return knn_grid_launch(nodes, n, k, max_dist, nbr, static_cast<char*>(ws), L, (hipStream_t)stream);
}

// Without a caller workspace: one cached workspace per device.  Reuse is ordered on the
// GPU (the next user's stream waits for the previous user's completion event), growth
// frees the old buffer only after the device drained it (hipFree synchronises).
epp_status epp_knn_grid(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* stream) {
    if (!knn_args_ok("epp_knn_grid", nodes, n, k, nbr)) return EPP_ERR_INVALID_ARGUMENT;
    if (n == 0) return EPP_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    CachedWs& c = g_knn_ws[dev & 63];
    std::lock_guard<std::mutex> lk(c.mu);
    hipStream_t s = (hipStream_t)stream;
    const KnnLayout L = knn_layout(n);
    const hipError_t e = c.acquire(s, L.bytes);
    if (e != hipSuccess) {
        set_error(std::string("epp_knn_grid: workspace: ") + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    const epp_status rc = knn_grid_launch(nodes, n, k, max_dist, nbr, static_cast<char*>(c.buf), L, s);
    c.release(s);
    return rc;
}

}  // extern "C"
