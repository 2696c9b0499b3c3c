// states_v4.hip — k_states_v4, the state check for worlds whose records, lists and class
// table together exceed k_states_v5's staging budget (states_kernels.h): records and lists in
// LDS where they fit, the class table read through L2.
#include "states_kernels.h"

namespace epp {
namespace {

// Fast-path parameters of the bitmap (kept in SGPRs; the rest of the WorldView is read
// through the scalar cache only on the rare exact path).
typedef const __attribute__((address_space(1))) uint16_t* gptr_u16;  // global, not flat

struct BmParams {
    gptr_u16 cls;
    float ox, oy, oz, ix, iy, iz;
    uint32_t nx, ny, nz, sentinel;
};

// index of the fine cell of p in cls[] (the zero sentinel when p is outside the grid)
__device__ __forceinline__ uint32_t cls_index(const BmParams& p, double px, double py, double pz) {
    const int ix = bm_axis(px, p.ox, p.ix), iy = bm_axis(py, p.oy, p.iy), iz = bm_axis(pz, p.oz, p.iz);
    const bool in = (unsigned)ix < p.nx && (unsigned)iy < p.ny && (unsigned)iz < p.nz;
    // dims <= 4096 per axis, so the products fit 24-bit multiplies
    const uint32_t c = __umul24(__umul24((uint32_t)iz, p.ny) + (uint32_t)iy, p.nx) + (uint32_t)ix;
    return in ? c : p.sentinel;
}

// 512 threads, two states per lane, high occupancy.  The states on occupied cells of the
// whole workgroup (~9% of 1024) are gathered into ONE LDS queue and tested by the first
// ceil(T/64) waves only, so the exact path runs on full wavefronts instead of ~10 active
// lanes in each of 8 waves.  Three barriers per item.
constexpr int kBlock4 = 512;
constexpr int kQueue4 = 2 * kBlock4;
struct StateQueue4 {
    double x[kQueue4], y[kQueue4], z[kQueue4];
    uint16_t cls[kQueue4];
    uint8_t hit[kQueue4];
    uint32_t wcnt[kBlock4 / 64];
};

// Block-wide copy of `bytes` (16-byte multiple) HBM -> LDS with global (not flat) loads,
// so waiting for the copy never waits on LDS traffic or vice versa.  No barrier.
__device__ __forceinline__ void stage_copy(unsigned char* dst, const unsigned char* src, uint32_t bytes,
                                           uint32_t nthreads) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(1))) uint4* gptr_u4;
    const gptr_u4 s = (gptr_u4)src;
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (uint32_t o = threadIdx.x; o < bytes / 16; o += nthreads) d[o] = s[o];
#endif
}

template <bool MINDIST, bool STAGE, bool COMPACT>
__global__ __launch_bounds__(kBlock4) void k_states_v4(const WorldView* __restrict__ wv,
                                                       const double* __restrict__ xyz, uint32_t items,
                                                       int64_t n, int can_pass, double md,
                                                       uint8_t* __restrict__ valid,
                                                       int32_t* __restrict__ compact_idx,
                                                       unsigned long long* __restrict__ n_valid,
                                                       uint32_t stage_bytes) {
    __shared__ StateQueue4 q;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_blob[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
    BmParams bp;
    bp.cls = (gptr_u16)(wv->blob + wv->off_bitmap);
    bp.ox = wv->bofx; bp.oy = wv->bofy; bp.oz = wv->bofz;
    bp.ix = wv->bix; bp.iy = wv->biy; bp.iz = wv->biz;
    bp.nx = (uint32_t)wv->bnx; bp.ny = (uint32_t)wv->bny; bp.nz = (uint32_t)wv->bnz;
    bp.sentinel = wv->bm_words;
    const uint32_t stride = gridDim.x * kBlock4;
    uint32_t it = blockIdx.x * kBlock4 + threadIdx.x;
    double v[6];
    auto load = [&](uint32_t i) {
        i = i < items ? i : items - 1;
        const double2* p = reinterpret_cast<const double2*>(xyz) + 3 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double2 t = p[k];
            v[2 * k] = t.x;
            v[2 * k + 1] = t.y;
        }
    };
    if (items > 0) load(it);
    // records + lists: [off_aos, off_pt) and [off_lists, off_bitmap) of the blob, staged into
    // LDS back to back (the point records between them stay behind)
    const uint32_t rec_bytes = wv->off_pt - wv->off_aos;
    const uint32_t lists_off = STAGE ? rec_bytes : wv->off_lists - wv->off_aos;
    const uint32_t ids_off = lists_off + (wv->off_ids - wv->off_lists);
    const uint32_t id_mask = wv->id_mask;
    const double rg = wv->r_gate, ro = wv->r_obst;
    const unsigned char* xbase;
    if (STAGE) {
        stage_copy(lds_blob, wv->blob + wv->off_aos, rec_bytes, kBlock4);
        stage_copy(lds_blob + rec_bytes, wv->blob + wv->off_lists, stage_bytes - rec_bytes, kBlock4);
        xbase = lds_blob;  // (the first barrier below orders the copy before any use)
    } else {
        xbase = wv->blob + wv->off_aos;
    }
    // block-uniform trip count: every thread runs every iteration (barriers)
    for (uint32_t i0 = blockIdx.x * kBlock4; i0 < items; i0 += stride, it += stride) {
        if (i0 != blockIdx.x * kBlock4) load(it);
        const bool live = it < items;
        const uint32_t c0 = bp.cls[cls_index(bp, v[0], v[1], v[2])];
        const uint32_t c1 = bp.cls[cls_index(bp, v[3], v[4], v[5])];
        const bool n0 = live & (c0 != 0u), n1 = live & (c1 != 0u);
        const unsigned long long b0 = __ballot(n0), b1 = __ballot(n1);
        const uint32_t t0 = (uint32_t)__popcll(b0), tw = t0 + (uint32_t)__popcll(b1);
        if (lane == 0) q.wcnt[wave] = tw;
        __syncthreads();
        // wave offset and block total (scalar loops over the 8 counters: no per-wave masks)
        uint32_t off = 0, T = 0;
        for (int w = 0; w < wave; ++w) off += q.wcnt[w];
        T = off;
        for (int w = wave; w < kBlock4 / 64; ++w) T += q.wcnt[w];
        uint32_t hits = 0;
        if (T > 0) {  // block-uniform
            const uint32_t p0 = off + lanes_below(b0), p1 = off + t0 + lanes_below(b1);
            if (n0) {
                q.x[p0] = v[0];
                q.y[p0] = v[1];
                q.z[p0] = v[2];
                q.cls[p0] = (uint16_t)c0;
            }
            if (n1) {
                q.x[p1] = v[3];
                q.y[p1] = v[4];
                q.z[p1] = v[5];
                q.cls[p1] = (uint16_t)c1;
            }
            __syncthreads();
            for (uint32_t e = threadIdx.x; e < T; e += kBlock4)  // only the first ceil(T/64) waves
                q.hit[e] = states_exact_rec<MINDIST>(xbase, lists_off, ids_off, id_mask, rg, ro, q.x[e], q.y[e], q.z[e], q.cls[e],
                                                     can_pass, md)
                               ? 1
                               : 0;
            __syncthreads();
            hits = (n0 && q.hit[p0] ? 1u : 0u) | (n1 && q.hit[p1] ? 2u : 0u);
        }
        const uint32_t fl = live ? (~hits & 3u) : 0u;
        if (live) *reinterpret_cast<uint16_t*>(valid + 2 * (size_t)it) = (uint16_t)((fl & 1u) | ((fl & 2u) << 7));
        if (COMPACT) compact_valid<2>(fl, 2 * (int64_t)it, lane, compact_idx, n_valid);
    }
    if (STAGE && items == 0) __syncthreads();  // (no loop ran: nothing read the copy)
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {  // odd last state
        const int64_t i = n - 1;
        const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
        const uint32_t c = bp.cls[cls_index(bp, px, py, pz)];
        const bool ok = !(c != 0u && states_exact_rec<MINDIST>(xbase, lists_off, ids_off, id_mask, rg, ro, px, py, pz, c, can_pass, md));
        valid[i] = ok ? 1 : 0;
        if (COMPACT && ok) compact_idx[atomicAdd(n_valid, 1ull)] = (int32_t)i;
    }
}

// k_states_v4 stages the records and the lists (not the point records between them)
uint32_t v4_staged(const WorldView& w) { return (w.off_pt - w.off_aos) + (w.off_bitmap - w.off_lists); }
bool v4_stage(const WorldView& w) { return v4_staged(w) + sizeof(StateQueue4) <= 160u * 1024u; }
// resident workgroups only (every block loops): LDS-limited, at most 3 per CU
int v4_grid(const WorldView& w, int64_t n) {
    const int64_t items = std::max<int64_t>(1, n / 2);
    const int64_t need = (items + kBlock4 - 1) / kBlock4;
    const uint32_t lds = sizeof(StateQueue4) + (v4_stage(w) ? v4_staged(w) : 0u);
    const int per_cu = std::max(1, std::min<int>(3, (int)((160u * 1024u) / lds)));
    const int64_t cap = (int64_t)cu_count() * per_cu;
    return (int)std::max<int64_t>(1, std::min(need, cap));
}

template <bool MINDIST>
void launch(const WorldView& w, const WorldView* dw, const double* xyz, int64_t n, int32_t can_pass, double md,
            uint8_t* valid, int32_t* compact_idx, unsigned long long* nv, hipStream_t st) {
    const uint32_t sb = v4_staged(w);
    const bool stg = v4_stage(w);
    const int g4 = v4_grid(w, n);
    const uint32_t items = (uint32_t)(n / 2);
#define EPP_LAUNCH_V4(S, C)                                                                                      \
    do {                                                                                                         \
        allow_lds(k_states_v4<MINDIST, S, C>, sizeof(StateQueue4));                                              \
        hipLaunchKernelGGL((k_states_v4<MINDIST, S, C>), dim3(g4), dim3(kBlock4), S ? sb : 0, st, dw, xyz, items, n, \
                           can_pass, md, valid, compact_idx, nv, sb);                                            \
    } while (0)
    if (compact_idx) {
        if (stg) EPP_LAUNCH_V4(true, true);
        else EPP_LAUNCH_V4(false, true);
    } else {
        if (stg) EPP_LAUNCH_V4(true, false);
        else EPP_LAUNCH_V4(false, false);
    }
#undef EPP_LAUNCH_V4
}

}  // namespace

bool states_v4_fits(const double* xyz, int64_t n, const uint8_t* valid) {
    return (reinterpret_cast<uintptr_t>(xyz) & 15) == 0 && (reinterpret_cast<uintptr_t>(valid) & 1) == 0 &&
           n / 2 < 0xFFFFFFFFll;
}

epp_status launch_states_v4(const WorldView& w, const WorldView* dw, bool mindist, const double* xyz, int64_t n,
                            int32_t can_pass, double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid,
                            hipStream_t st, const char* what) {
    auto nv = reinterpret_cast<unsigned long long*>(n_valid);
    if (mindist) launch<true>(w, dw, xyz, n, can_pass, md, valid, compact_idx, nv, st);
    else launch<false>(w, dw, xyz, n, can_pass, md, valid, compact_idx, nv, st);
    return launch_error(what);
}

}  // namespace epp
