// planner.hip — the small stages of the planner that replaces OMPL's RRT*/FMT* driver behind
// PathPlanner::planPath (src/PathPlanner.cpp:80-158), and their entry points:
//
//   k_sample_uniform            : counter-based uniform state sampler (splitmix64)
//                                 -- the state sampler OMPL's RealVectorStateSpace would provide
//   k_compact                   : ordered compaction of the valid states (decoupled look-back)
//   k_knn_edges                 : gathers the candidate edges (node, neighbour) for the motion check
//   k_mask_edges[_count]        : drops the edges the motion check refused (and counts the rest)
//   k_rev_count / scan / fill / sort : the reverse edges of a k-NN table as a CSR
//
// The k-NN itself is knn*.hip (knn_kernels.h), the batched planner plan_batch.hip; both use the scan tag
// handed out here (planner_common.h).  States and edges are checked by the states_*.hip and
// motions_*.hip kernels; the host runs the shortest-path search over the valid edges.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>

#include "cached_ws.h"
#include "epp_internal.h"
#include "planner_common.h"

namespace epp {

namespace {
std::atomic<uint32_t> g_scan_tag{0};
}
uint32_t next_scan_tag() {
    uint32_t t;
    do t = (g_scan_tag.fetch_add(1, std::memory_order_relaxed) + 1u) & 0xffffffu;
    while (t == 0u);
    return t;
}

namespace {

// (clr, nclr: words a later kernel on the stream needs zeroed, cleared here instead of by a
// separate fill launch; epp_sample_uniform passes none)
__global__ void k_sample_uniform(uint64_t seed, double lox, double loy, double loz, double hix,
                                 double hiy, double hiz, int64_t n, int64_t start,
                                 double* __restrict__ xyz, unsigned long long* __restrict__ clr, int64_t nclr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nclr) clr[i] = 0ull;
    if (i >= n) return;
    const double lo[3] = {lox, loy, loz}, hi[3] = {hix, hiy, hiz};
    sample_uniform(seed, (uint64_t)(start + i), lo, hi, xyz + 3 * i);
}

__global__ void k_knn_edges(const double* __restrict__ nodes, const int32_t* __restrict__ nbr, int64_t m,
                            int k, double* __restrict__ s1, double* __restrict__ s2) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const int64_t i = e / k;
    const int32_t j = nbr[e];
    const int64_t jj = j < 0 ? i : j;  // missing neighbour: a degenerate edge
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        s1[3 * e + d] = nodes[3 * i + d];
        s2[3 * e + d] = nodes[3 * jj + d];
    }
}

CachedWs g_compact_ws[64];

// ---- ordered compaction of the valid states ----------------------------------------
// One pass: block b owns states [b C, (b+1) C) (C = kCompactChunk) in kCompactRounds rounds
// of one state per thread (coalesced flag loads and row copies); ranks from wave ballots
// and the per-(round, wave) counts in LDS, the block's offset by look-back.  The valid
// states are written in index order.  Deterministic: the planner's node order (and with
// it k-NN tie breaks and the search) does not depend on scheduling.

// (block b of nb; the last block writes *n_out = the valid count + add)
__device__ __forceinline__ void compact_block(const double* __restrict__ xyz, const uint8_t* __restrict__ valid,
                                              int64_t n, unsigned long long* __restrict__ st, uint32_t tag,
                                              double* __restrict__ out, int64_t* __restrict__ n_out, int64_t add,
                                              const int b, const int nb) {
    constexpr int NW = kCompactThreads / 64;
    __shared__ int wcnt[kCompactRounds * NW];
    __shared__ long long s_excl;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)b * kCompactChunk + threadIdx.x;
    bool v[kCompactRounds];
    unsigned long long bal[kCompactRounds];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const int64_t i = i0 + r * kCompactThreads;
        v[r] = i < n && valid[i] != 0;
    }
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        bal[r] = __ballot(v[r]);
        if (lane == 0) wcnt[r * NW + wv] = __popcll(bal[r]);
    }
    __syncthreads();
    // (round, wave) slots in index order: round-major
    int before[kCompactRounds], total = 0;
#pragma unroll
    for (int q = 0; q < kCompactRounds * NW; ++q) {
#pragma unroll
        for (int r = 0; r < kCompactRounds; ++r)
            if (q == r * NW + wv) before[r] = total;
        total += wcnt[q];
    }
    if (wv == 0) {
        if (lane == 0) lb_publish(st, b, tag, b == 0, total);
        const long long ex = b == 0 ? 0ll : lb_exclusive(st, b, tag);
        if (lane == 0) {
            if (b > 0) lb_publish(st, b, tag, true, ex + total);
            s_excl = ex;
            if (b == nb - 1) *n_out = ex + total + add;
        }
    }
    __syncthreads();
    const long long ex = s_excl;
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        if (v[r]) {
            const int64_t i = i0 + r * kCompactThreads;
            const int64_t p = ex + before[r] +
                              (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal[r] >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)bal[r], 0u));
            out[3 * p] = xyz[3 * i];
            out[3 * p + 1] = xyz[3 * i + 1];
            out[3 * p + 2] = xyz[3 * i + 2];
        }
    }
}
__global__ __launch_bounds__(kCompactThreads) void k_compact(const double* __restrict__ xyz,
                                                             const uint8_t* __restrict__ valid, int64_t n,
                                                             unsigned long long* __restrict__ st, uint32_t tag,
                                                             double* __restrict__ out, int64_t* __restrict__ n_out) {
    compact_block(xyz, valid, n, st, tag, out, n_out, 0, blockIdx.x, gridDim.x);
}

__global__ void k_mask_edges(int32_t* __restrict__ nbr, const uint8_t* __restrict__ valid, int64_t m) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < m && !valid[e]) nbr[e] = -1;
}

// The same, plus count[0] += the surviving edges (entries >= 0 after masking) and
// count[1] += the surviving edges into node `target`.  Grid-stride over at most one
// 1024-thread block per CU, wave popcounts, one atomic per block and counter (an atomic
// per 256 edges put thousands on one address: ~45 us for 1M edges).
constexpr int kMaskThreads = 1024;
__global__ __launch_bounds__(kMaskThreads) void k_mask_edges_count(int32_t* __restrict__ nbr,
                                                                   const uint8_t* __restrict__ valid, int64_t m,
                                                                   int32_t target,
                                                                   unsigned long long* __restrict__ count,
                                                                   uint16_t* __restrict__ out16) {
    __shared__ uint32_t part[2][kMaskThreads / 64];
    uint32_t c = 0, ci = 0;
    for (int64_t e = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; e < m;
         e += (int64_t)gridDim.x * kMaskThreads) {  // (uniform trip count per wave but the last)
        const int32_t v = nbr[e];
        const bool ok = valid[e] != 0;
        if (!ok) nbr[e] = -1;
        const bool keep = ok && v >= 0;
        if (out16) out16[e] = keep ? (uint16_t)v : (uint16_t)0xFFFF;  // (a narrow copy for the download)
        c += keep ? 1u : 0u;
        ci += (keep && v == target) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        c += (uint32_t)__shfl_xor((int)c, o, 64);
        ci += (uint32_t)__shfl_xor((int)ci, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = c;
        part[1][threadIdx.x >> 6] = ci;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t t = 0;
        for (int w = 0; w < kMaskThreads / 64; ++w) t += part[threadIdx.x][w];
        if (t) atomicAdd(count + threadIdx.x, (unsigned long long)t);
    }
}

// ---- the reverse edges of a k-NN table as a CSR (the planner's symmetrised search) -----
// roff[v] .. roff[v + 1]: the nodes u whose (masked) row holds v, ascending -- the order
// the host's own build gives them (rows scanned in node order), so A* relaxes them in the
// same order.  Counting sort: in-degrees by atomics, one workgroup's scan, a scatter by
// atomics, then every node's run sorted (insertion sort: ~k entries).
__global__ __launch_bounds__(256) void k_rev_count(const int32_t* __restrict__ nbr, int64_t m, int32_t* __restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < m && nbr[e] >= 0) atomicAdd(&cnt[nbr[e]], 1);
}
__global__ __launch_bounds__(1024) void k_rev_scan(const int32_t* __restrict__ cnt, int32_t n, int32_t* __restrict__ roff,
                                                   int32_t* __restrict__ fill) {
    __shared__ int wsum[16];
    __shared__ int s_carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    for (int c0 = 0; c0 < n; c0 += 1024 * 16) {  // chunks of 16 counts per thread
        const int b0 = c0 + (int)threadIdx.x * 16;
        int v[16], sum = 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            v[u] = b0 + u < n ? cnt[b0 + u] : 0;
            sum += v[u];
        }
        int incl = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        __syncthreads();
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int acc = s_carry + incl - sum;
        for (int w = 0; w < wv; ++w) acc += wsum[w];
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = acc + sum;
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (b0 + u < n) {
                roff[b0 + u] = acc;
                fill[b0 + u] = acc;
                acc += v[u];
            }
    }
    __syncthreads();
    if (threadIdx.x == 0) roff[n] = s_carry;
}
__global__ __launch_bounds__(256) void k_rev_fill(const int32_t* __restrict__ nbr, int64_t m, int32_t k,
                                                  int32_t* __restrict__ fill, int32_t* __restrict__ radj) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int32_t v = nbr[e];
    if (v >= 0) radj[atomicAdd(&fill[v], 1)] = (int32_t)(e / k);
}
__global__ __launch_bounds__(256) void k_rev_sort(const int32_t* __restrict__ roff, int32_t n, int32_t* __restrict__ radj,
                                                  uint16_t* __restrict__ radj16) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int a = roff[v], b = roff[v + 1];
    for (int i = a + 1; i < b; ++i) {  // (insertion sort of the node's run)
        const int32_t x = radj[i];
        int j = i - 1;
        while (j >= a && radj[j] > x) {
            radj[j + 1] = radj[j];
            --j;
        }
        radj[j + 1] = x;
    }
    if (radj16)
        for (int i = a; i < b; ++i) radj16[i] = (uint16_t)radj[i];
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_sample_uniform(uint64_t seed, const double lo[3], const double hi[3], int64_t n,
                              int64_t start, double* xyz, void* stream) {
    if (n < 0 || (n > 0 && (!lo || !hi || !xyz))) {
        set_error("epp_sample_uniform: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    hipLaunchKernelGGL(k_sample_uniform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       seed, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], n, start, xyz, nullptr, (int64_t)0);
    return launch_error("epp_sample_uniform");
}

epp_status epp_compact_states(const double* xyz, const uint8_t* valid, int64_t n, double* out, int64_t* n_out,
                              void* stream) {
    if (n < 0 || !n_out || (n > 0 && (!xyz || !valid || !out))) {
        set_error("epp_compact_states: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    // the look-back status words live in a cached per-device workspace (stream-ordered reuse)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    CachedWs& c = g_compact_ws[dev & 63];
    std::lock_guard<std::mutex> lk(c.mu);
    hipError_t e = c.acquire(s, (size_t)epp_compact_workspace_size(n));
    if (e != hipSuccess) {
        set_error(std::string("epp_compact_states: workspace: ") + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    const epp_status rc = epp_compact_states_ws(xyz, valid, n, out, n_out, c.buf, c.cap, stream);
    c.release(s);
    return rc;
}

uint64_t epp_compact_workspace_size(int64_t n) {
    return n <= 0 ? 8 : (uint64_t)((n + kCompactChunk - 1) / kCompactChunk) * 8;
}

epp_status epp_compact_states_ws(const double* xyz, const uint8_t* valid, int64_t n, double* out, int64_t* n_out,
                                 void* ws, uint64_t ws_bytes, void* stream) {
    if (n < 0 || !n_out || (n > 0 && (!xyz || !valid || !out)) || !ws || ws_bytes < epp_compact_workspace_size(n) ||
        (reinterpret_cast<uintptr_t>(ws) & 7)) {
        set_error("epp_compact_states: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    const int nb = (int)std::max<int64_t>(1, (n + kCompactChunk - 1) / kCompactChunk);
    // the workspace may hold anything (e.g. carved from a buffer that held other data):
    // zero its status words first, so none reads as published in this launch
    if (hipMemsetAsync(ws, 0, (size_t)nb * 8, (hipStream_t)stream) != hipSuccess) return launch_error("epp_compact_states");
    hipLaunchKernelGGL(k_compact, dim3(nb), dim3(kCompactThreads), 0, (hipStream_t)stream, xyz, valid, n,
                       static_cast<unsigned long long*>(ws), next_scan_tag(), out, n_out);
    return launch_error("epp_compact_states");
}

epp_status epp_mask_edges(int32_t* nbr, const uint8_t* valid, int64_t m, void* stream) {
    if (m < 0 || (m > 0 && (!nbr || !valid))) {
        set_error("epp_mask_edges: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (m == 0) return EPP_OK;
    hipLaunchKernelGGL(k_mask_edges, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nbr,
                       valid, m);
    return launch_error("epp_mask_edges");
}

epp_status epp_mask_edges_count(int32_t* nbr, const uint8_t* valid, int64_t m, int32_t target, int64_t* count,
                                void* stream) {
    if (m < 0 || !count || (m > 0 && (!nbr || !valid))) {
        set_error("epp_mask_edges_count: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (hipMemsetAsync(count, 0, 2 * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return launch_error("epp_mask_edges_count");
    return epp::mask_edges_count_acc(nbr, valid, m, target, count, stream);
}

}  // extern "C"

epp_status epp::mask_edges_count_acc(int32_t* nbr, const uint8_t* valid, int64_t m, int32_t target, int64_t* count,
                                     void* stream, uint16_t* out16) {
    if (m < 0 || !count || (m > 0 && (!nbr || !valid))) {
        set_error("epp_mask_edges_count: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) return EPP_OK;
    const int64_t blocks = std::min<int64_t>((m + kMaskThreads - 1) / kMaskThreads, 256);
    hipLaunchKernelGGL(k_mask_edges_count, dim3((unsigned)blocks), dim3(kMaskThreads), 0, s, nbr, valid, m, target,
                       reinterpret_cast<unsigned long long*>(count), out16);
    return launch_error("epp_mask_edges_count");
}

extern "C" {

epp_status epp_knn_edges(const double* nodes, const int32_t* nbr, int32_t n, int32_t k, double* s1,
                         double* s2, void* stream) {
    if (n < 0 || k <= 0 || (n > 0 && (!nodes || !nbr || !s1 || !s2))) {
        set_error("epp_knn_edges: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    const int64_t m = (int64_t)n * k;
    if (m == 0) return EPP_OK;
    hipLaunchKernelGGL(k_knn_edges, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nodes,
                       nbr, m, k, s1, s2);
    return launch_error("epp_knn_edges");
}

}  // extern "C"

epp_status epp::reverse_csr(const int32_t* nbr, int32_t n, int32_t k, int32_t* cnt, int32_t* fill, int32_t* roff,
                            int32_t* radj, uint16_t* radj16, void* stream) {
    if (n <= 0 || k <= 0 || !nbr || !cnt || !fill || !roff || !radj) {
        set_error("reverse_csr: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t m = (int64_t)n * k;
    if (hipMemsetAsync(cnt, 0, (size_t)n * 4, s) != hipSuccess) return launch_error("reverse_csr");
    hipLaunchKernelGGL(k_rev_count, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, nbr, m, cnt);
    hipLaunchKernelGGL(k_rev_scan, dim3(1), dim3(1024), 0, s, cnt, n, roff, fill);
    hipLaunchKernelGGL(k_rev_fill, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, nbr, m, k, fill, radj);
    hipLaunchKernelGGL(k_rev_sort, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, roff, n, radj, radj16);
    return launch_error("reverse_csr");
}
