// states_kernels.h — batched state validity checks for gfx950 (MI355X).
//
//   World::checkPointValidity(p, canPassGate)  src/World.cpp:80-104
//   World::checkPointValidity(p, minDistance)  src/World.cpp:106-128  (MINDIST)
//   + optional wave-ballot compaction of the valid states (no reference counterpart)
//
// Kernels, tried in this order by epp_check_states[_mindist] (states.hip), first fit wins:
//   k_states_small  batches of <= 4096 states on worlds of <= 256 OBBs            small.hip
//   k_states_v5     default: records + lists + fine-cell class table staged in LDS, one
//                   class lookup per state, exact fp64 tests only for the ~10% of states
//                   whose class cell some inflated AABB reaches                   states_v5.hip
//   k_states_v4     worlds whose staged part exceeds kStageBudget (e.g. C3's 512 OBBs):
//                   class table read through L2, records + lists in LDS           states_v4.hip
//   k_states        generic: any world size, unaligned buffers (coarse grid walk) states_generic.hip
// Layout: a lane owns consecutive states (96 B = six 16-B loads for four) and writes their
// flag bytes with one store.
//
// The kernels sit in anonymous namespaces, so each file offers a host launcher and, where its
// kernel does not take every call, the predicate that says whether it takes this one.  A
// launcher enqueues on st and returns the launch status (launch_error(what)).  A
// -DEPP_STATES_TL build adds a per-wave timeline to k_states_v5 (states_diag.h).
#pragma once
#include "collision_common.h"

namespace epp {

// (states_v5.hip) the staged part fits the LDS budget, xyz is 16-byte and valid 4-byte aligned
bool states_v5_fits(const WorldView& w, bool mindist, const double* xyz, int64_t n, const uint8_t* valid);
epp_status launch_states_v5(const WorldView& w, bool mindist, const double* xyz, int64_t n, int32_t can_pass,
                            double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid, hipStream_t st,
                            const char* what);

// (states_v4.hip) xyz is 16-byte and valid 2-byte aligned, the state pairs fit 32 bits
bool states_v4_fits(const double* xyz, int64_t n, const uint8_t* valid);
epp_status launch_states_v4(const WorldView& w, const WorldView* dw, bool mindist, const double* xyz, int64_t n,
                            int32_t can_pass, double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid,
                            hipStream_t st, const char* what);

// (states_generic.hip) fits every world and every buffer
epp_status launch_states_generic(const WorldView& w, bool mindist, const double* xyz, int64_t n, int32_t can_pass,
                                 double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid, hipStream_t st,
                                 const char* what);

namespace {

// bits 0-3 of fl as four flag bytes (one 32-bit store writes a lane's four states)
__device__ __forceinline__ uint32_t pack_flags4(uint32_t fl) {
    return (fl & 1u) | ((fl & 2u) << 7) | ((fl & 4u) << 14) | ((fl & 8u) << 21);
}

// Wave-ballot compaction, called by every lane of the wave: bit k of fl says that the lane's
// state first + k (k < PER_LANE) is valid.  The wave takes its share of compact_idx with one
// atomic and each lane appends its valid states' indices.
template <int PER_LANE>
__device__ __forceinline__ void compact_valid(uint32_t fl, int64_t first, int lane, int32_t* __restrict__ compact_idx,
                                              unsigned long long* __restrict__ n_valid) {
    const uint32_t c = (uint32_t)__popc(fl);
    uint32_t ctot;
    const uint32_t cex = wave_excl_scan(c, lane, ctot);
    unsigned long long wbase = 0;
    if (lane == 0 && ctot) wbase = atomicAdd(n_valid, (unsigned long long)ctot);
    wbase = __shfl(wbase, 0, 64);
    uint64_t pos = wbase + cex;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k)
        if ((fl >> k) & 1u) compact_idx[pos++] = (int32_t)(first + k);
}

// Exact test on the AoS records + the cell's candidate list (no early exit: the lists
// are short and straight-line control flow keeps the wave converged).  `sbase` points
// at the records (LDS copy or HBM); `lists_off` / `ids_off` are relative to it.
// (id_mask: WorldView::id_mask, the list ids less their filling flag)
template <bool MINDIST>
__device__ __forceinline__ bool states_exact_rec(const unsigned char* sbase, uint32_t lists_off, uint32_t ids_off,
                                                 uint32_t id_mask, double rg, double ro, double px, double py,
                                                 double pz, uint32_t cls, int can_pass, double md) {
    const double* recs = reinterpret_cast<const double*>(sbase);
    const uint32_t h = reinterpret_cast<const uint32_t*>(sbase + lists_off)[cls];
    const uint16_t* ids = reinterpret_cast<const uint16_t*>(sbase + ids_off) + (h >> 12);
    const uint32_t cnt = h & 4095u;
    bool hit = false;
    for (uint32_t j = 0; j < cnt; ++j)
        hit |= rec_hit<MINDIST>(recs + (size_t)(ids[j] & id_mask) * kRecDoubles, rg, ro, px, py, pz, can_pass != 0, md);
    return hit;
}

}  // namespace
}  // namespace epp
