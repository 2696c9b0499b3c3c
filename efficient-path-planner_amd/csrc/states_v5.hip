// states_v5.hip — k_states_v5, the default state check (states_kernels.h) and the project's
// headline kernel: the whole decision runs out of LDS.
//
// Persistent workgroups (one per CU), four states per lane (96 B = six 16-B loads),
// the next group prefetched while the current one is classified.  The world's
// records, candidate lists and fine-cell class table are staged into LDS once per
// workgroup while the first group's HBM loads are in flight.  Per state: class lookup
// (LDS, ~15 VALU: the class grid's empty margin cells make a clamp do the bounds test)
// -> ballot; a group with needy states queues them in the wave's LDS queue and, in the
// common case (<= 64 needy states and <= 128 candidate pairs), tests each (state,
// candidate) pair on its own lane (the pairs laid out by a lane permute and a max-scan, no
// LDS round trip) with the hits returned by one ballot per 64 pairs; otherwise each
// queued state walks its own list.  One 32-bit store writes a lane's four flags.
// The per-state VALU count matters: at 1M states/launch the kernel's critical path is
// the last-arriving data plus the VALU work behind it (PMC: SQ_INSTS_VALU).
#include "states_diag.h"
#include "states_kernels.h"

namespace epp {
namespace {

// States per lane and group.  (Eight per lane, i.e. fewer waves and fewer executions of the
// per-wave fixed costs, was measured and lost: DESIGN.md §4.)
constexpr int kStatesPerLane = 4;

struct WaveQueue5 {
    double x[64], y[64], z[64];
    uint32_t hdr[64];  // the queued states' list headers (start << 12 | count)
};
template <int BLOCK>
constexpr uint32_t queue5_bytes() { return (BLOCK / 64) * sizeof(WaveQueue5); }

// hardware f32 -> i32 conversion (NaN -> 0, saturating), then clamp to [0, n-1]
__device__ __forceinline__ uint32_t cell_axis5(double p, float off, float inv, uint32_t nm1) {
    const float f = fmaf((float)p, inv, off);
    int i;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(i) : "v"(f));
    return min((uint32_t)i, nm1);  // negative -> huge -> last (empty) cell
}
// a * b + c on 24-bit operands (cells per axis <= 4096), b wave-uniform: one v_mad_u32_u24
// (__umul24(a, b) + c becomes a 64-bit v_mad_u64_u32)
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}
// The (state, candidate) pairs of a queue round are laid out over the lanes by a forward
// lane permute (ds_permute_b32: no LDS memory is touched).  Lane i sends `data` to lane
// `target` (mod 64); a lane that no lane targets receives 0.  Every lane of the wave
// executes it (a lane outside EXEC would neither send nor receive); where several lanes
// target one lane the callers make them send the same value, so the result does not depend
// on which of them the hardware lets win.
__device__ __forceinline__ uint32_t lane_scatter(uint32_t target, uint32_t data) {
    return (uint32_t)__builtin_amdgcn_ds_permute((int)((target & 63u) << 2), (int)data);
}

// rec_hit<false> on a point record (epp_internal.h: kPtDoubles; `pts` the first record, `ide`
// a list id with its filling flag, worlds with WorldView::id_mask = 0x7FFF only): the record
// is seven aligned 16-byte reads, the thresholds tx ty tz come inflated from the host (the
// same IEEE additions and selects, so the same doubles), and "filling" from the id's bit 15:
// no meta word, no radius select, no additions.  The same conjunction of fp64 comparisons in
// the same arithmetic (no contraction: -ffp-contract=off), so the booleans are rec_hit's.
__device__ __forceinline__ bool point_rec_hit(const unsigned char* pts, uint32_t ide, double px, double py, double pz,
                                              bool can_pass) {
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const uint32_t i = ide & (kIdFill - 1u);
    f64x2 q[7];
#pragma unroll
    for (uint32_t k = 0; k < 7; ++k) q[k] = *reinterpret_cast<const f64x2*>(pts + pt_chunk_off(i, k));
    const double lox = q[0].x, loy = q[0].y, loz = q[1].x, hix = q[1].y, hiy = q[2].x, hiz = q[2].y;
    const double cx = q[3].x, cy = q[3].y, cz = q[4].x, c = q[4].y, s = q[5].x;
    const double tx = q[5].y, ty = q[6].x, tz = q[6].y;
    // rtree contains(point): strict  src/World.cpp:83
    const bool in = (lox < px) & (px < hix) & (loy < py) & (py < hiy) & (loz < pz) & (pz < hiz);
    const bool skip = ((ide & kIdFill) != 0u) & can_pass;  // :92-95
    // OBB::checkCollisionWithPoint — src/OBB.cpp:63-91 (same evaluation as obb_point_hit)
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    const double lx = c * dx + s * dy;
    const double ly = c * dy - s * dx;
    return in & !skip & (fabs(lx) <= tx) & (fabs(ly) <= ty) & (fabs(dz) <= tz);
}

// states_exact_rec<false> on the point records: `sbase` points at them (LDS copy or HBM).
__device__ __forceinline__ bool states_exact_pt(const unsigned char* sbase, uint32_t lists_off, uint32_t ids_off,
                                                double px, double py, double pz, uint32_t cls, int can_pass) {
    const uint32_t h = reinterpret_cast<const uint32_t*>(sbase + lists_off)[cls];
    const uint16_t* ids = reinterpret_cast<const uint16_t*>(sbase + ids_off) + (h >> 12);
    const uint32_t cnt = h & 4095u;
    bool hit = false;
    for (uint32_t j = 0; j < cnt; ++j) hit |= point_rec_hit(sbase, ids[j], px, py, pz, can_pass != 0);
    return hit;
}

#ifdef EPP_STATES_TL
__device__ unsigned long long g_states_tl[kTlWaves][kTlWords];  // the last launch's timeline (states_diag.h)
#endif

// The world's parameters reach the kernel by value (V5Args, filled on the host by
// v5_args): nothing on a wave's way to its first load or to the staging barrier is
// fetched through a pointer into device memory.  The arguments the first loads need
// (stage_src = blob + off_pt, or + off_aos for MINDIST; xyz, groups, stage_bytes) lead the list, scalars and
// pointers only, so that the kernel-argument preload (Makefile, STATES_PRELOAD) delivers
// them in SGPRs at wave launch; the struct comes last (a leading struct disables the
// preload).
struct V5Args {
    uint32_t lists_off, ids_off;  // list headers / list ids, bytes from the staged copy's start
    uint32_t cls_off, cls_nz_off;  // the class table (bytes or u16) / the sparse classes' bytes
    uint32_t nx, ny, nz;          // class cells per axis
    float ox, oy, oz, ix, iy, iz;  // cell coordinate f = fmaf((float)p, i, o)
    // (no inflate radii: the plain test's thresholds come inflated in the point records, the
    // MINDIST one inflates by its own argument)
};

// PREFETCH: groups per lane > 1 (the next group's loads overlap this one's work);
// single-pass launches (e.g. 1M states on 256 CUs) drop the second buffer's registers.
// SC: staging chunks (16 B) per lane: enough for the staged bytes (launcher's choice).
// The single-pass 512-thread shape (the headline's) is held to five waves per SIMD's worth of
// registers (96 VGPRs), as it was built before the lane-permute pair layout; no scratch
// (tests/test_kernel_resources.py).
template <bool MINDIST, bool COMPACT, int BLOCK, bool PREFETCH, bool C8, int SC>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BLOCK == 512 && !PREFETCH ? 5 : BLOCK / 256)))
void k_states_v5(const unsigned char* stage_src, const double* xyz,
                                                     int64_t groups, uint32_t stage_bytes, int can_pass,
                                                     int64_t n, double md, uint8_t* __restrict__ valid,
                                                     int32_t* __restrict__ compact_idx,
                                                     unsigned long long* __restrict__ n_valid, V5Args wa) {
    __shared__ WaveQueue5 queues[BLOCK / 64];
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_blob[];
    const int lane = threadIdx.x & 63;
    EPP_STL(0);
    WaveQueue5* qu = &queues[threadIdx.x >> 6];
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    const int64_t gfirst = (int64_t)blockIdx.x * BLOCK;
    int64_t g = gfirst + threadIdx.x;
    constexpr int NV = 3 * kStatesPerLane;  // doubles per group
    double va[NV], vb[NV];
    // (no full group: loads read the staging source instead, >= 16 * NV / 2 bytes
    // (states_v5_fits checks), ignored)
    const double* xyzb = groups > 0 ? xyz : reinterpret_cast<const double*>(stage_src);
    auto load = [&](int64_t grp, double (&dst)[NV]) {
        grp = grp < groups ? grp : groups - 1;
        grp = grp < 0 ? 0 : grp;
        const double2* q = reinterpret_cast<const double2*>(xyzb) + (NV / 2) * grp;
#pragma unroll
        for (int k = 0; k < NV / 2; ++k) {
            const double2 t = q[k];
            dst[2 * k] = t.x;
            dst[2 * k + 1] = t.y;
        }
    };
    // [off_pt, ...): point records, list headers, list ids, class table (MINDIST: from off_aos,
    // the 17-double records first, the point records riding along unused).  The copy's
    // loads are issued BEFORE the group's loads and stored after them, so the stores
    // wait on a counted vmcnt that leaves the group's HBM loads in flight, and the
    // barrier below never waits on HBM.  Every lane loads and stores every chunk slot
    // (clamped source; out-of-range chunks go to a dummy LDS slot): no branches.  xyz
    // is not __restrict__ so its loads cannot be sunk past the LDS stores.
    // (LDS-DMA variants were tried: hipcc then drains vmcnt at the first use of any
    // group, prefetched ones included.)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // (HIP's uint4 struct ends up on the stack)
    constexpr int kStageChunks = SC;
    u32x4 stg[kStageChunks];
    const uint32_t n16 = stage_bytes / 16u;  // >= 1 (the class table's sentinel)
#if defined(__HIP_DEVICE_COMPILE__)  // global (not flat) loads: flat ones would also count lgkmcnt and force vmcnt(0)
    typedef const __attribute__((address_space(1))) u32x4* gptr_stage;
    const gptr_stage ssrc = (gptr_stage)stage_src;
#else
    const u32x4* ssrc = reinterpret_cast<const u32x4*>(stage_src);
#endif
#pragma unroll
    for (int i = 0; i < kStageChunks; ++i) {
        const uint32_t o = (uint32_t)(i * BLOCK) + threadIdx.x;
        stg[i] = ssrc[o < n16 ? o : n16 - 1u];
    }
    load(g, va);  // unconditional (clamped): a branch here would make hipcc's vmcnt counts conservative
#pragma unroll
    for (int i = 0; i < kStageChunks; ++i) {
        const uint32_t o = (uint32_t)(i * BLOCK) + threadIdx.x;
        // (the launch allocates 16 spare bytes after the copy: the dummy slot)
        *reinterpret_cast<u32x4*>(lds_blob + 16u * (o < n16 ? o : n16)) = stg[i];
    }
    const uint32_t lists_off = wa.lists_off, ids_off = wa.ids_off;
    // the class table: bytes (C8, staged right after the lists) or u16
    const unsigned char* cls_base = lds_blob + wa.cls_off;
    [[maybe_unused]] const unsigned char* cls_nz = lds_blob + wa.cls_nz_off;  // (sparse classes)
    const uint32_t* hdrs = reinterpret_cast<const uint32_t*>(lds_blob + lists_off);
    const uint16_t* ids_all = reinterpret_cast<const uint16_t*>(lds_blob + ids_off);
    const float ox = wa.ox, oy = wa.oy, oz = wa.oz, ix = wa.ix, iy = wa.iy, iz = wa.iz;
    const uint32_t nx = wa.nx, ny = wa.ny, nz = wa.nz;
    __syncthreads();
    EPP_STL(1);
    // One (state, candidate) test; `ide`: the list's id entry (bit 15 = filling).  The staged
    // copy starts with the records the instantiation tests on: the point records (plain) or
    // the 17-double records (MINDIST: its radius is md, the world's radii are not used).
    auto hit_of = [&](uint32_t ide, double px, double py, double pz) -> bool {
        if constexpr (MINDIST)
            return rec_hit<true>(reinterpret_cast<const double*>(lds_blob) + (size_t)(ide & (kIdFill - 1u)) * kRecDoubles,
                                 0.0, 0.0, px, py, pz, false, md);
        else
            return point_rec_hit(lds_blob, ide, px, py, pz, can_pass != 0);
    };
    auto cell_of = [&](double px, double py, double pz) -> uint32_t {
        const uint32_t cx = cell_axis5(px, ox, ix, nx - 1), cy = cell_axis5(py, oy, iy, ny - 1),
                       cz = cell_axis5(pz, oz, iz, nz - 1);
        return mad_u24(mad_u24(cz, ny, cy), nx, cx);
    };
    // Classes of N cells, batched and branch-free: all the first reads are issued, then all
    // the second ones, so N lookups cost two LDS round trips (sparse bytes) or one, not
    // 2 N.  occ[k] != 0: the class is not 0 — for sparse bytes that is the cell's occupancy
    // bit, known one round trip before c[k].
    // Sparse byte classes: per 32 cells one u64 [occupancy bits | occupied cells before this
    // word], then the class bytes (all non-zero) of the occupied cells.  The class byte is
    // read for every cell, occupied or not, and dropped for an unoccupied one.  There
    // rank <= the number of occupied cells, so the read may land on the first byte after
    // the class bytes, at cls_nz_off + occupied = cls_off + cls8_bytes <= stage_bytes
    // (v5_staged rounds that end up to 16): inside the launch's stage_bytes + 16 bytes
    // of dynamic LDS (launch, dyn), at worst in the staging copy's dummy slot.
    auto classes_of = [&](const auto& idx, auto& c, auto& occ) {
        constexpr int N = (int)(sizeof(idx) / sizeof(idx[0]));
        if (C8) {
            uint64_t wd[N];
            uint32_t rank[N];
#pragma unroll
            for (int k = 0; k < N; ++k) wd[k] = reinterpret_cast<const uint64_t*>(cls_base)[idx[k] >> 5];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const uint32_t m = (uint32_t)wd[k], sh = idx[k] & 31u;
                rank[k] = (uint32_t)(wd[k] >> 32) + (uint32_t)__popc(m & ((1u << sh) - 1u));
                occ[k] = (m >> sh) & 1u;
            }
#pragma unroll
            for (int k = 0; k < N; ++k) c[k] = (uint32_t)cls_nz[rank[k]];
#pragma unroll
            for (int k = 0; k < N; ++k) c[k] = occ[k] ? c[k] : 0u;
            return;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            c[k] = (uint32_t)reinterpret_cast<const uint16_t*>(cls_base)[idx[k]];  // (u16 classes)
            occ[k] = c[k];
        }
    };
#ifdef EPP_STATES_TL
    uint32_t tl_needy = 0, tl_pairs = 0;  // (diagnostics) queued states and pairs
#endif
    auto process = [&](int64_t gg, const double (&v)[NV]) {
        const bool live = gg < groups;
        uint32_t c[kStatesPerLane];
        bool needy[kStatesPerLane];
        unsigned long long b[kStatesPerLane];
        uint32_t base[kStatesPerLane], total = 0;
#ifdef EPP_STATES_TL
        if (!PREFETCH) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            EPP_STL(2);
        }
#endif
        uint32_t cell[kStatesPerLane], occ[kStatesPerLane];
#pragma unroll
        for (int k = 0; k < kStatesPerLane; ++k) cell[k] = cell_of(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
        classes_of(cell, c, occ);
        const uint32_t live_bits = live ? ~0u : 0u;
#pragma unroll
        for (int k = 0; k < kStatesPerLane; ++k) {
            // (one compare: its lane mask is the ballot)
            needy[k] = (occ[k] & live_bits) != 0u;
            b[k] = __builtin_amdgcn_ballot_w64(needy[k]);
            base[k] = total;
            total += (uint32_t)__popcll(b[k]);
        }
        EPP_STL(3);
        // the needy states' list headers, read now (one LDS round trip for all four,
        // overlapping the ballot arithmetic) and queued with the state
        uint32_t hd[kStatesPerLane];
#pragma unroll
        for (int k = 0; k < kStatesPerLane; ++k) hd[k] = hdrs[needy[k] ? c[k] : 0u];  // list 0 is empty
        uint32_t hits = 0;
#ifdef EPP_STATES_NOEXACT  // diagnostics builds only (wrong answers): the cost of the exact path
#pragma unroll
        for (int k = 0; k < kStatesPerLane; ++k) hits |= needy[k] ? 1u << k : 0u;
        if (false) {
#else
        if (total > 0) {  // wave-uniform
#endif
            uint32_t pos[kStatesPerLane];
#pragma unroll
            for (int k = 0; k < kStatesPerLane; ++k) pos[k] = base[k] + lanes_below(b[k]);
            // queue the needy states (slot = rank in the wave), rounds of 64
            for (uint32_t r0 = 0; r0 < total; r0 += 64) {
#pragma unroll
                for (int k = 0; k < kStatesPerLane; ++k) {
                    const uint32_t slot = pos[k] - r0;
                    if (needy[k] && slot < 64u) {
                        qu->x[slot] = v[3 * k];
                        qu->y[slot] = v[3 * k + 1];
                        qu->z[slot] = v[3 * k + 2];
                        qu->hdr[slot] = hd[k];
                    }
                }
                wave_lds_sync();
                const uint32_t tq = min(total - r0, 64u);
                // lane e < tq owns queued state e: its candidate list
                const bool act = (uint32_t)lane < tq;
                const uint32_t hq = act ? qu->hdr[lane] : 0u;
                const uint32_t cnt = hq & 4095u, first = hq >> 12;
                uint32_t ptot;
                const uint32_t poff = wave_excl_scan(cnt, lane, ptot);
#ifdef EPP_STATES_TL
                tl_needy += tq;
                tl_pairs += ptot;
#endif
                bool hit_e = false;
                if (ptot <= 128u) {
                    // one (state, candidate) pair per lane and round (two rounds at most):
                    // state e marks pair position poff_e, the head of its segment (distinct
                    // positions: cnt >= 1 for queued states), with
                    //   (e + 1) << 21 | (first_e - poff_e + 128)
                    // (first: 20 bits, poff <= 128, so the low field is < 2^21 and not
                    // negative; e + 1 <= 64), sent there by one lane_scatter per 64 positions.
                    // The max-scan of the heads hands pair q its state (the high field
                    // orders the heads) and, in the low field, its id's index less q - 128.
                    // Hits come back by ballot.
                    // Lanes with no head among the 64 positions repeat a head that is: lane
                    // 0's (position 0) for the first 64, the last queued state's for the
                    // second 64 (poff ascends: if its head is not there, no head is, and
                    // everyone sends 0).
                    uint32_t ln = (uint32_t)lane;
                    asm volatile("" : "+v"(ln));  // (keeps (lane + 1) << 21 from living in a register of its own)
                    const uint32_t head = (ln << 21) + (first - poff + ((1u << 21) + 128u));
                    const bool own0 = act & (poff < 64u);
                    const uint32_t head0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)head);
                    const uint32_t h0 = dpp_incl_max(lane_scatter(own0 ? poff : 0u, own0 ? head : head0));
                    auto test = [&](uint32_t h, uint32_t q) {
                        const uint32_t e = (h >> 21) - 1u;  // (h != 0: position 0 is a head)
                        return q < ptot && hit_of(ids_all[(h & 0x1FFFFFu) + q - 128u], qu->x[e], qu->y[e], qu->z[e]);
                    };
                    unsigned long long m1 = 0ull;
                    uint32_t h1 = 0u;
                    if (ptot > 64u) {  // wave-uniform
                        const uint32_t plast = (uint32_t)__builtin_amdgcn_readlane((int)poff, (int)(tq - 1u));
                        const uint32_t hlast = (uint32_t)__builtin_amdgcn_readlane((int)head, (int)(tq - 1u));
                        const bool own1 = act & (poff >= 64u);
                        const uint32_t carry = (uint32_t)__builtin_amdgcn_readlane((int)h0, 63);
                        h1 = max(dpp_incl_max(lane_scatter(own1 ? poff : plast,  // (mod 64)
                                                           own1 ? head : (plast >= 64u ? hlast : 0u))),
                                 carry);
                    }
                    const unsigned long long m0 = __builtin_amdgcn_ballot_w64(test(h0, (uint32_t)lane));
                    if (ptot > 64u) m1 = __builtin_amdgcn_ballot_w64(test(h1, 64u + (uint32_t)lane));
                    // any hit among this state's pairs [poff, poff + cnt) of the 128-bit mask
                    auto bits = [](unsigned long long m, uint32_t from, uint32_t len) {
                        const unsigned long long msk = len >= 64u ? ~0ull : ((1ull << len) - 1ull);
                        return ((m >> from) & msk) != 0ull;
                    };
                    const uint32_t end = poff + cnt;
                    const bool lo = poff < 64u && bits(m0, poff, min(end, 64u) - poff);
                    const bool hi = end > 64u && bits(m1, poff > 64u ? poff - 64u : 0u, end - max(poff, 64u));
                    hit_e = act && (lo || hi);
                } else if (act) {  // long lists: each queued state walks its own
                    const uint16_t* idl = reinterpret_cast<const uint16_t*>(lds_blob + ids_off) + first;
                    const double px = qu->x[lane], py = qu->y[lane], pz = qu->z[lane];
                    for (uint32_t j = 0; j < cnt; ++j) hit_e |= hit_of(idl[j], px, py, pz);
                }
                // back to the owners: state slot r0 + e lives on lane e
                const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit_e);
#pragma unroll
                for (int k = 0; k < kStatesPerLane; ++k) {
                    const uint32_t slot = pos[k] - r0;
                    if (needy[k] && slot < 64u && ((hm >> slot) & 1ull)) hits |= 1u << k;
                }
                wave_lds_sync();  // the queue is rewritten next
            }
        }
        EPP_STL(4);
        const uint32_t fl = live ? (~hits & ((1u << kStatesPerLane) - 1u)) : 0u;  // bit k: state 4 gg + k valid
        if (live) *reinterpret_cast<uint32_t*>(valid + kStatesPerLane * gg) = pack_flags4(fl);
        if (COMPACT) compact_valid<kStatesPerLane>(fl, kStatesPerLane * gg, lane, compact_idx, n_valid);
    };
    // block-uniform trip count; the next group's loads are issued before this one is
    // classified (vmcnt counts in order: the class lookups never wait on them)
    if (PREFETCH) {  // prefetch loads unconditional (clamped): counted vmcnt, no merge points
        for (int64_t g0 = gfirst; g0 < groups; g0 += 2 * stride, g += 2 * stride) {
            load(g + stride, vb);
            process(g, va);
            if (g0 + stride >= groups) break;
            load(g + 2 * stride, va);
            process(g + stride, vb);
        }
    } else {
        for (int64_t g0 = gfirst; g0 < groups; g0 += stride, g += stride) {
            if (g0 != gfirst) load(g, va);
            process(g, va);
        }
    }
#ifdef EPP_STATES_TL
    EPP_STL(5);
    if (lane == 0) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        const int w_ = (int)((blockIdx.x * BLOCK + threadIdx.x) >> 6);
        if (w_ < kTlWaves)
            g_states_tl[w_][6] = hw | ((unsigned long long)min(tl_needy, 65535u) << 32) |
                                 ((unsigned long long)min(tl_pairs, 65535u) << 48);
    }
#endif
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - kStatesPerLane * groups)) {  // tail: the last n % 4 states
        const int64_t i = kStatesPerLane * groups + threadIdx.x;
        const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
        const uint32_t cell[1] = {cell_of(px, py, pz)};
        uint32_t c[1], occ[1];
        classes_of(cell, c, occ);
        bool hit = false;
        if (occ[0] != 0u) {
            if constexpr (MINDIST)
                hit = states_exact_rec<true>(lds_blob, lists_off, ids_off, kIdFill - 1u, 0.0, 0.0, px, py, pz, c[0], 0, md);
            else
                hit = states_exact_pt(lds_blob, lists_off, ids_off, px, py, pz, c[0], can_pass);
        }
        const bool ok = !hit;
        valid[i] = ok ? 1 : 0;
        if (COMPACT && ok) compact_idx[atomicAdd(n_valid, 1ull)] = (int32_t)i;
    }
}

// ---- launch ---------------------------------------------------------------------------
// k_states_v5 stages records, lists and the class table (bytes when there are, else u16):
// [start, end of the byte table) or [start, blob_bytes), from the point records on (plain) or
// from the 17-double records on (MINDIST: the point records in between are copied with them)
uint32_t v5_start(const WorldView& w, bool mindist) { return mindist ? w.off_aos : w.off_pt; }
uint32_t v5_staged(const WorldView& w, bool mindist) {
    return (w.off_cls8 ? ((w.off_cls8 + w.cls8_bytes + 15u) & ~15u) : w.blob_bytes) - v5_start(w, mindist);
}
// The by-value world parameters of k_states_v5 (offsets relative to the staged copy)
V5Args v5_args(const WorldView& w, bool mindist) {
    V5Args a{};
    const uint32_t start = v5_start(w, mindist);
    a.lists_off = w.off_lists - start;
    a.ids_off = w.off_ids - start;
    a.cls_off = (w.off_cls8 ? w.off_cls8 : w.off_bitmap) - start;
    a.cls_nz_off = a.cls_off + ((w.bm_words + 1u + 31u) >> 5) * 8u;
    a.nx = (uint32_t)w.bnx; a.ny = (uint32_t)w.bny; a.nz = (uint32_t)w.bnz;
    a.ox = w.bofx; a.oy = w.bofy; a.oz = w.bofz;
    a.ix = w.bix; a.iy = w.biy; a.iz = w.biz;
    return a;
}
// Launches without a full group (n < 4) aim their (ignored) state loads at the staging
// source: it must hold the 96 bytes a lane loads.
constexpr uint32_t kV5DummyBytes = 96;
// (the list ids carry the filling flag the point test needs: id_mask; always so for a world
// that fits, <= 512 OBBs)
bool v5_fits(const WorldView& w, bool mindist) {
    const uint32_t sb = v5_staged(w, mindist);
    return sb <= kStageBudget && sb + 16u + queue5_bytes<1024>() <= 160u * 1024u && w.id_mask == kIdFill - 1u;
}

// Launch shape of k_states_v5.  Single pass (every lane one group, e.g. 1M states on 256
// CUs): two 512-thread workgroups per CU when two staged copies fit in LDS (1M states:
// 8.3-8.4 us vs 8.7-8.8 us for one 1024-thread workgroup — each half of the CU syncs and
// stages on its own), else one 1024-thread workgroup.  More than one pass: one 512-thread
// workgroup per CU, the next group prefetched.  Test hook (not for production use):
// EPP_V5_BLOCK = 256 | 512 | 1024 forces the workgroup size (256: single pass only, and 512
// takes its place when compaction is asked for), so every shape can be checked against the
// oracle.
struct V5Shape {
    int64_t gN;
    int bs, grid;
    bool pf;
};
V5Shape v5_shape(int64_t n, uint32_t sb) {
    V5Shape r{};
    const int64_t cus = cu_count();
    r.gN = n / kStatesPerLane;
    const int forced = env_int("EPP_V5_BLOCK", 0);
    if (forced == 256 && 4u * (sb + 16u + queue5_bytes<256>()) <= 160u * 1024u && r.gN <= 4 * cus * 256) {
        // (test hook / A/B) single pass on four 256-thread workgroups per CU
        r.bs = 256;
        r.grid = (int)std::max<int64_t>(1, (r.gN + 255) / 256);
        r.pf = false;
        return r;
    }
    const bool two = forced == 0 && 2u * (sb + 16u + queue5_bytes<512>()) <= 160u * 1024u && r.gN <= 2 * cus * 512;
    if (two) {
        r.bs = 512;
        r.grid = (int)std::max<int64_t>(1, (r.gN + 511) / 512);
        r.pf = false;
        return r;
    }
    const bool single = r.gN <= cus * 1024;
    r.bs = forced == 512 ? 512 : forced == 1024 ? 1024 : (single ? 1024 : 512);
    r.grid = (int)std::max<int64_t>(1, std::min<int64_t>((r.gN + r.bs - 1) / r.bs, cus));
    r.pf = r.gN > (int64_t)r.grid * r.bs;  // more than one group per lane
    return r;
}

template <bool MINDIST>
void launch(const WorldView& w, const double* xyz, int64_t n, int32_t can_pass, double md, uint8_t* valid,
            int32_t* compact_idx, unsigned long long* nv, hipStream_t st) {
    const uint32_t sb = v5_staged(w, MINDIST);
    V5Shape sh = v5_shape(n, sb);
    if (sh.bs == 256 && compact_idx) {  // (the 256-thread shape is instantiated without compaction)
        sh.bs = 512;
        sh.grid = (int)std::max<int64_t>(1, (sh.gN + 511) / 512);
    }
    const uint32_t dyn = sb + 16u;  // the staged world + the dummy slot of the copy
    const unsigned char* src = w.blob + v5_start(w, MINDIST);
    const V5Args wa = v5_args(w, MINDIST);
#define EPP_LAUNCH_V5S(C, B, P, C8, SC)                                                                           \
    do {                                                                                                          \
        allow_lds(k_states_v5<MINDIST, C, B, P, C8, SC>, queue5_bytes<B>());                                      \
        hipLaunchKernelGGL((k_states_v5<MINDIST, C, B, P, C8, SC>), dim3(sh.grid), dim3(B), dyn, st, src, xyz,   \
                           sh.gN, sb, can_pass, n, md, valid, compact_idx, nv, wa);                               \
    } while (0)
    // staging chunks per lane: as many as the staged bytes need (1, 2 or 3), else half
    // the budget's or the whole budget's
    const bool half_stage = sb <= (uint32_t)kStageBudget / 2;
#define EPP_LAUNCH_V5C(C, B, P, C8)                                                              \
    do {                                                                                         \
        if (sb <= (uint32_t)B * 16u) EPP_LAUNCH_V5S(C, B, P, C8, 1);                              \
        else if (sb <= (uint32_t)B * 32u) EPP_LAUNCH_V5S(C, B, P, C8, 2);                         \
        else if (sb <= (uint32_t)B * 48u) EPP_LAUNCH_V5S(C, B, P, C8, 3);                         \
        else if (half_stage) EPP_LAUNCH_V5S(C, B, P, C8, (int)(kStageBudget / 2 / (B * 16)));    \
        else EPP_LAUNCH_V5S(C, B, P, C8, (int)(kStageBudget / (B * 16)));                        \
    } while (0)
#define EPP_LAUNCH_V5(C, B, P)                                 \
    do {                                                       \
        if (w.off_cls8) EPP_LAUNCH_V5C(C, B, P, true);          \
        else EPP_LAUNCH_V5C(C, B, P, false);                    \
    } while (0)
#define EPP_LAUNCH_V5B(B)                                \
    do {                                                 \
        if (sh.pf) {                                     \
            if (compact_idx) EPP_LAUNCH_V5(true, B, true);  \
            else EPP_LAUNCH_V5(false, B, true);          \
        } else {                                         \
            if (compact_idx) EPP_LAUNCH_V5(true, B, false); \
            else EPP_LAUNCH_V5(false, B, false);         \
        }                                                \
    } while (0)
    if (sh.bs == 256) EPP_LAUNCH_V5(false, 256, false);  // (EPP_V5_BLOCK=256, single pass)
    else if (sh.bs == 512) EPP_LAUNCH_V5B(512);
    else EPP_LAUNCH_V5B(1024);
#undef EPP_LAUNCH_V5B
#undef EPP_LAUNCH_V5
#undef EPP_LAUNCH_V5C
#undef EPP_LAUNCH_V5S
}

}  // namespace

bool states_v5_fits(const WorldView& w, bool mindist, const double* xyz, int64_t n, const uint8_t* valid) {
    return v5_fits(w, mindist) && (reinterpret_cast<uintptr_t>(xyz) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(valid) & 3) == 0 &&
           (n >= kStatesPerLane || w.blob_bytes - v5_start(w, mindist) >= kV5DummyBytes);
}

epp_status launch_states_v5(const WorldView& w, bool mindist, const double* xyz, int64_t n, int32_t can_pass,
                            double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid, hipStream_t st,
                            const char* what) {
    auto nv = reinterpret_cast<unsigned long long*>(n_valid);
    if (mindist) launch<true>(w, xyz, n, can_pass, md, valid, compact_idx, nv, st);
    else launch<false>(w, xyz, n, can_pass, md, valid, compact_idx, nv, st);
    return launch_error(what);
}

}  // namespace epp

#ifdef EPP_STATES_TL
// diagnostics builds only: the per-wave timeline of the last k_states_v5 launch
extern "C" epp_status epp_dbg_states_tl(unsigned long long* out, int64_t waves) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(epp::g_states_tl),
                               (size_t)std::min<int64_t>(waves, epp::kTlWaves) * epp::kTlWords * 8) == hipSuccess
               ? EPP_OK
               : EPP_ERR_HIP;
}
#endif
