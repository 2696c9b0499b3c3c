// motions_kernels.h — batched motion (edge) validity checks for gfx950 (MI355X).
//
//   World::checkRayValid(s, e, canPassGate)  src/World.cpp:130-162, via
//   OBB::checkCollisionWithRay               src/OBB.cpp:10-61        (mode 0, analytic)
//   32-step discretised check                BASELINE config 3         (mode 1; points
//   s + (e - s) k/32, k = 1..32, each World::checkPointValidity(p, canPassGate))
//
// Kernels, tried in this order by epp_check_motions (motions.hip), first fit wins:
//   k_motions_small  batches of <= 1024 edges on worlds of <= 256 OBBs          small.hip
//   k_motions_v5     both modes, tile/slab bit-set candidate filter (records and
//                    tile rows in LDS; worlds of <= 1024 OBBs per tile) — the
//                    default, and the only one the k-NN-table entries use        motions_tile.hip
//   k_motions_v4     analytic, coarse grid + records in LDS, lane-balanced walk  motions_cells.hip
//   k_motions_d32b   discrete32, same staging, lane-balanced walk per step       motions_cells.hip
//   k_motions        generic (worlds too large for LDS): one lane per edge,
//                    L2-resident world                                           motions_generic.hip
//
// The kernels sit in anonymous namespaces, so each file offers a host launcher.  A launcher
// enqueues on st and returns true, or returns false with nothing launched when the world
// does not fit its kernel; the caller reads the launch status (launch_error()).  A
// -DEPP_MOTIONS_TL build adds per-wave timelines to the tile and cell-list kernels
// (motions_diag.h, scripts/motions_timeline.py).
#pragma once
#include <hip/hip_runtime.h>

#include "epp_internal.h"

namespace epp {

// (motions_tile.hip) nbr == nullptr: the edges s1[i] -> s2[i]; else the k-NN table nbr
// (rows of kk entries over the nodes s1; s2 unused), optionally with the planner's mask mm.
bool launch_motions_tile(const WorldView* dw, const WorldView& w, const double* s1, const double* s2,
                         const int32_t* nbr, int kk, int64_t n, int32_t can_pass_gate, int32_t mode, uint8_t* valid,
                         hipStream_t st, const MotionMask& mm = MotionMask{});
// whether launch_motions_tile would launch: tile tables exist and fit the LDS budget
bool motions_tile_fits(const WorldView& w);

// (motions_cells.hip) k_motions_v4 (mode 0) or k_motions_d32b (mode 1)
bool launch_motions_cells(const WorldView* dw, const WorldView& w, const double* s1, const double* s2, int64_t n,
                          int32_t can_pass_gate, int32_t mode, uint8_t* valid, hipStream_t st);

// (motions_generic.hip) fits every world
void launch_motions_generic(const WorldView& w, const double* s1, const double* s2, int64_t n, int32_t can_pass_gate,
                            int32_t mode, uint8_t* valid, hipStream_t st);

}  // namespace epp
