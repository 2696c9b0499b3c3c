// states_generic.hip — k_states, the state check that fits every world and every buffer
// (states_kernels.h): the coarse grid walked per state, the world in LDS as far as it fits.
#include "states_kernels.h"

namespace epp {
namespace {

// ---- k_states: wave-cooperative candidate testing ----------------------------------
// Phase 1 (per lane, 4 states): bounds + fine-mask test.  A state whose sub-cell is
// occupied owns a segment of (state, candidate OBB) pairs: its coarse cell's list.
// Phase 2 (per wave): the segments are compacted into LDS (wave prefix sums) and the 64
// lanes take one pair each (a binary search over the segment offsets finds the pair's
// state), setting per-state "hit" bits with LDS atomics.  Only ~6% of uniform samples
// have candidates; without this a wavefront would run its slowest lane's candidate loop
// for every state slot.
constexpr int kSegCap = 96;     // needy states a wave handles cooperatively per group
constexpr int kPairCap = 512;   // (state, candidate) pairs a wave handles cooperatively
struct WaveScratch {
    double xyz[kSegCap][3];        // coordinates of the needy states
    uint32_t seg_start[kSegCap];   // exclusive prefix of pair counts
    uint32_t seg_state[kSegCap];   // sid (8 bits) | first candidate entry << 8
    uint8_t head[kPairCap];        // segment index at its first pair, 0 elsewhere
    uint32_t bits[8];              // hit bits of the 256 states of the wave's group
};
constexpr uint32_t kScratchBytes = (kBlock / 64) * ((sizeof(WaveScratch) + 15) & ~15u);

// STAGE: 0 = world read from HBM/L2, 1 = front (masks, cell starts) in LDS, 2 = all in LDS
template <int STAGE, bool MINDIST, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void k_states(WorldView w, const double* __restrict__ xyz,
                                                   int64_t n, int can_pass, double md,
                                                   uint8_t* __restrict__ valid,
                                                   int32_t* __restrict__ compact_idx,
                                                   unsigned long long* __restrict__ n_valid,
                                                   uint32_t stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = threadIdx.x & 63;
    // full groups of 4 states; the (< 4) tail states are handled after the main loop
    const int64_t groups = n / 4;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // Loads are unconditional (clamped to the last full group) so the compiler keeps
    // the next group's six loads in flight with a counted vmcnt.
    auto load = [&](int64_t grp, double (&dst)[12]) {
        grp = grp < groups ? grp : groups - 1;
        if (ALIGNED) {
            const double2* q = reinterpret_cast<const double2*>(xyz + 12 * grp);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double2 t = q[k];
                dst[2 * k] = t.x;
                dst[2 * k + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) dst[k] = xyz[12 * grp + k];
        }
    };
    int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double va[12], vb[12];
    if (groups > 0) load(g, va);  // first loads before the world staging
    WaveScratch* ws = reinterpret_cast<WaveScratch*>(lds + (threadIdx.x >> 6) * ((sizeof(WaveScratch) + 15) & ~15u));
    const unsigned char* staged = STAGE ? stage_world(w, lds + kScratchBytes, stage_bytes) : w.blob;
    const Acc a = make_acc(staged, STAGE == 2 ? staged : w.blob, w);

    auto process = [&](int64_t gg, const double (&v)[12]) {
        const bool live = gg < groups;
        const int64_t first = 4 * gg;
        // phase 1
        uint32_t cst[4], cnt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = classify(a, w, v[3 * k], v[3 * k + 1], v[3 * k + 2], cst[k]);
            cnt[k] = live ? c : 0u;
        }
        const uint32_t mine = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        const uint32_t nseg = (cnt[0] > 0) + (cnt[1] > 0) + (cnt[2] > 0) + (cnt[3] > 0);
        uint32_t total, S;
        const uint32_t pexcl = wave_excl_scan(mine, lane, total);
        const uint32_t sexcl = wave_excl_scan(nseg, lane, S);
        uint32_t hits = 0;
        if (total && S <= (uint32_t)kSegCap && total <= (uint32_t)kPairCap) {
            // wave-uniform: cooperative pair testing.  Pair p belongs to the last segment
            // starting at or before p: heads are scattered to LDS and propagated with a
            // wave max-scan (carried across rounds), no search.
            if (lane < 8) ws->bits[lane] = 0;
            for (uint32_t p = lane; p < total; p += 64) ws->head[p] = 0;
            wave_lds_sync();
            uint32_t si = sexcl, pp = pexcl;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cnt[k]) {
                    ws->seg_start[si] = pp;
                    ws->seg_state[si] = (uint32_t)(lane * 4 + k) | (cst[k] << 8);
                    ws->xyz[si][0] = v[3 * k];
                    ws->xyz[si][1] = v[3 * k + 1];
                    ws->xyz[si][2] = v[3 * k + 2];
                    ws->head[pp] = (uint8_t)si;
                    ++si;
                    pp += cnt[k];
                }
            wave_lds_sync();
            uint32_t carry = 0;
            for (uint32_t r = 0; r < total; r += 64) {  // wave-uniform rounds
                const uint32_t p = r + lane;
                const uint32_t hd = p < total ? (uint32_t)ws->head[p] : 0u;
                const uint32_t j = max(dpp_incl_max(hd), carry);
                carry = (uint32_t)__builtin_amdgcn_readlane((int)j, 63);
                if (p < total) {
                    const uint32_t e = ws->seg_state[j];
                    const int i = a.co[(e >> 8) + (p - ws->seg_start[j])];
                    if (pair_hit<MINDIST>(a, w, i, ws->xyz[j][0], ws->xyz[j][1], ws->xyz[j][2],
                                          can_pass != 0, md)) {
                        const uint32_t sid = e & 255u;
                        atomicOr(&ws->bits[sid >> 5], 1u << (sid & 31));
                    }
                }
            }
            wave_lds_sync();
            hits = (ws->bits[lane >> 3] >> ((lane & 7) * 4)) & 15u;
            wave_lds_sync();  // scratch is rewritten by the next group
        } else if (total) {  // rare: too many needy states, every lane walks its own lists
#pragma unroll
            for (int k = 0; k < 4; ++k)
                for (uint32_t j = 0; j < cnt[k]; ++j)
                    if (pair_hit<MINDIST>(a, w, a.co[cst[k] + j], v[3 * k], v[3 * k + 1], v[3 * k + 2],
                                          can_pass != 0, md)) {
                        hits |= 1u << k;
                        break;
                    }
        }
        const uint32_t fl = live ? (~hits & 15u) : 0u;  // bit k: state first+k valid
        if (live) {
            if (ALIGNED)
                *reinterpret_cast<uint32_t*>(valid + first) = pack_flags4(fl);
            else
                for (int k = 0; k < 4; ++k) valid[first + k] = (uint8_t)((fl >> k) & 1u);
        }
        if (compact_idx) compact_valid<4>(fl, first, lane, compact_idx, n_valid);  // (uniform branch)
    };
    // block-uniform trip count: every lane runs every iteration (ballots, wave scratch);
    // ping-pong register buffers: the next group loads while this one is processed
    for (int64_t g0 = (int64_t)blockIdx.x * kBlock; g0 < groups; g0 += 2 * stride, g += 2 * stride) {
        load(g + stride, vb);
        process(g, va);
        if (g0 + stride >= groups) break;
        load(g + 2 * stride, va);
        process(g + stride, vb);
    }
    // tail: the last n % 4 states, one lane each
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * groups)) {
        const int64_t i = 4 * groups + threadIdx.x;
        const bool ok = state_valid_scalar<MINDIST>(a, w, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2],
                                                    can_pass != 0, md);
        valid[i] = ok ? 1 : 0;
        if (compact_idx && ok) compact_idx[atomicAdd(n_valid, 1ull)] = (int32_t)i;
    }
}

template <bool MINDIST>
void launch(const WorldView& w, const double* xyz, int64_t n, int32_t can_pass, double md, uint8_t* valid,
            int32_t* compact_idx, unsigned long long* nv, hipStream_t st) {
    // stage the whole world when it is small (several blocks per CU), else only the front
    // (occupancy masks + cell starts) and read the OBB table through L1/L2
    const bool aligned = (reinterpret_cast<uintptr_t>(xyz) & 15) == 0 && (reinterpret_cast<uintptr_t>(valid) & 3) == 0;
    const bool lds = w.front_bytes + kScratchBytes <= kLdsBudget;
    const uint32_t stage = !lds ? 0u : (w.blob_bytes <= 40u * 1024u ? w.blob_bytes : w.front_bytes);
    const uint32_t shm = kScratchBytes + stage;
    const int grid = grid_for(std::max<int64_t>(1, n / 4), shm);
#define EPP_LAUNCH_STATES(L, A)                                                                              \
    do {                                                                                                     \
        allow_lds(k_states<L, MINDIST, A>);                                                                  \
        hipLaunchKernelGGL((k_states<L, MINDIST, A>), dim3(grid), dim3(kBlock), shm, st, w, xyz, n, can_pass, md, \
                           valid, compact_idx, nv, stage);                                                   \
    } while (0)
    const int mode = stage == 0 ? 0 : (stage == w.blob_bytes ? 2 : 1);
    if (mode == 2 && aligned) EPP_LAUNCH_STATES(2, true);
    else if (mode == 2) EPP_LAUNCH_STATES(2, false);
    else if (mode == 1 && aligned) EPP_LAUNCH_STATES(1, true);
    else if (mode == 1) EPP_LAUNCH_STATES(1, false);
    else if (aligned) EPP_LAUNCH_STATES(0, true);
    else EPP_LAUNCH_STATES(0, false);
#undef EPP_LAUNCH_STATES
}

}  // namespace

epp_status launch_states_generic(const WorldView& w, bool mindist, const double* xyz, int64_t n, int32_t can_pass,
                                 double md, uint8_t* valid, int32_t* compact_idx, int64_t* n_valid, hipStream_t st,
                                 const char* what) {
    auto nv = reinterpret_cast<unsigned long long*>(n_valid);
    if (mindist) launch<true>(w, xyz, n, can_pass, md, valid, compact_idx, nv, st);
    else launch<false>(w, xyz, n, can_pass, md, valid, compact_idx, nv, st);
    return launch_error(what);
}

}  // namespace epp
