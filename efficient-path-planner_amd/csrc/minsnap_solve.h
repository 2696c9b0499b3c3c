// minsnap_solve.h — the minimum-snap solve of one track by one workgroup, for gfx950: the
// device code the batch fit (minsnap.hip, k_minsnap) and the single-track latency path
// (minsnap_refit.hip, k_refit / k_check_refit) share, and the constants it reads.
//
// Reference: poly_traj::generateTrajectory (external/poly_traj/src/trajectory_generator.cpp:12-100)
// built on mav_trajectory_generation::PolynomialOptimization<10>
// (include/mav_trajectory_generation/impl/polynomial_optimization_linear_impl.h).
//
// The formulation is the reference's:
//   T_i      Nfabian segment times                          src/vertex.cpp:272-289
//   A_i^-1   Schur inverse of the mapping matrix             impl :111-121, :142-179
//   Q_i      snap cost matrix                                impl :567-583
//   H_i      = A_i^-T Q_i A_i^-1                             impl :307-336
//   R_pp d_p = -R_pf d_f                                     impl :338-379
//   p_i      = A_i^-1 [d(vertex i); d(vertex i+1)]           impl :262-283
// The free constraints are derivatives 1..4 of the inner vertices, so R_pp is
// block-tridiagonal with 4x4 blocks (vertex v couples only with v-1 and v+1).  It is
// SPD and solved by block elimination (block Thomas with explicit 4x4 inverses) instead
// of the reference's Eigen SparseQR/COLAMD; the two agree to rounding (parity target 1e-6).
//
// Everything here sits in the anonymous namespace, and the library is not built as
// relocatable device code: every translation unit that includes this header has its own
// copy of the constants (cC) and fills it at its own first use (ensure_consts, which each
// launcher of such a unit calls before its launch).  That is intended: the kernels read cC
// as before the units were split, so their code is what it was.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "epp_internal.h"
#include "minsnap_consts.h"
#include "minsnap_diag.h"
#include "traj_sample.h"

namespace epp {
namespace {

constexpr int N = 10;
constexpr int HALF = 5;
constexpr int kWave = 64;

// The kernels' constants, one block (kNC doubles, set once per device by ensure_consts and
// staged into LDS at kernel entry, overlapping the inputs' loads — lane-indexed reads of
// __constant__ memory are vector loads that miss the caches on the latency path):
//   kCB   falling factorials B[k][j] = j! / (j-k)!  (src/polynomial.cpp:145-160), 10 x 10
//   kCB5  B5^-1, kCK  K, 5 x 5 each: the constants of the closed-form mapping inverse
//         (see hess and phase 4 of solve_track)
//   kCF   1 / r!, r = 0..4
//   kCH   Hc, the constant part of H = A^-T Q A^-1 (hess below), 10 x 10
constexpr int kCB = 0, kCB5 = 100, kCK = 125, kCF = 150, kCH = 156, kNC = 256;  // (kNC even: 16-byte aligned LDS after it)
__constant__ double cC[kNC];
template <int BLOCK>
__device__ __forceinline__ void stage_consts(double* dst) {
    for (int e = threadIdx.x; e < kNC; e += BLOCK) dst[e] = cC[e];
}

// Fills this translation unit's cC on the current device, once per device.
bool g_consts_ready[64];
epp_status ensure_consts() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && g_consts_ready[dev]) return EPP_OK;
    // B5^-1, K and Hc (see hess): exact rationals rounded once to double (minsnap_consts.h,
    // scripts/gen_minsnap_consts.py).
    // (Round 5 derived them here in long double; Hc's products cancel, and some entries
    // were ~3e-13 off -- data error the solve amplified to ~1e-9 in the coefficients.)
    double cc[kNC] = {};
    for (int k = 0; k < N; ++k)
        for (int j = 0; j < N; ++j) cc[kCB + k * N + j] = falling_factorial(k, j);  // (traj_sample.h)
    for (int r = 0; r < HALF; ++r)
        for (int c = 0; c < HALF; ++c) {
            cc[kCB5 + r * HALF + c] = minsnap_consts::kB5inv[r * HALF + c];
            cc[kCK + r * HALF + c] = minsnap_consts::kK[r * HALF + c];
        }
    const double inv_fact[HALF] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0};
    for (int r = 0; r < HALF; ++r) cc[kCF + r] = inv_fact[r];
    for (int i = 0; i < N * N; ++i) cc[kCH + i] = minsnap_consts::kHc[i];
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(cC), cc, sizeof(cc));
    if (e != hipSuccess) {
        set_error(std::string("epp minsnap: constants: ") + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    if (dev >= 0 && dev < 64) g_consts_ready[dev] = true;
    return EPP_OK;
}

// Workgroup barrier.  SCR_LDS (all the solve's shared data in LDS): waits for this
// wave's LDS operations only, so global loads issued earlier (e.g. the refit's host
// reads of its sample data) stay in flight across it; else a full __syncthreads.
template <bool SCR_LDS>
__device__ __forceinline__ void block_sync() {
    if (SCR_LDS) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
}

// Orders one wavefront's LDS accesses across its lanes (LDS operations of a wavefront
// complete in order; this waits for them and stops the compiler moving memory accesses
// across the point).
__device__ __forceinline__ void wave_sync_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// setupMappingMatrix + invertMappingMatrix (impl :111-121, :142-179) in closed form.  The
// mapping matrix is A = [[diag(k!), 0], [C, D]] with C[k][j] = B[k][j] T^(j-k) and
// D[k][j] = B[k][j+5] T^(j+5-k), i.e. D = diag(T^-k) B5 diag(T^(j+5)) for the constant
// B5[k][j] = B[k][j+5].  So
//   A^-1 = [[diag(1/k!), 0], [-D^-1 C diag(1/k!), D^-1]],
//   D^-1[r][c] = B5^-1[r][c] T^(c-r-5),   (-D^-1 C diag(1/k!))[r][c] = K[r][c] T^(c-r-5)
// with constant B5^-1 and K[r][c] = -sum_{k<=c} B5^-1[r][k] B[k][c] / c!: every entry is
// a constant times a power of 1/T, so the 100 entries are independent (one thread each)
// instead of a 5x5 LU per segment on one lane.  The reference's LU with partial pivoting
// gives the same matrix to rounding (the parity target of the solve is 1e-6).  Phase 4 of
// solve_track applies these rows (kCF, kCK, kCB5 and the segment's powers of 1/T) directly.

// H_i = A_i^-T Q_i A_i^-1 in closed form.  Row a >= 4 of A^-1 is a constant times
// T^(c%5 - a) in column c (the closed form above), and Q[a][b] (a, b >= 4) a constant times
// T^(a+b-7) (computeQuadraticCostJacobian, impl :567-583), so every term of
//   H[r][c] = sum_{a,b >= 4} A^-1[a][r] Q[a][b] A^-1[b][c]
// carries the same power T^((r%5) + (c%5) - 7): H[r][c] = Hc[r][c] T^((r%5) + (c%5) - 7)
// with the constant Hc (computed once on the host in long double, kCH).  The solve
// reads the H entries it needs straight from Hc and the powers of T: no per-segment
// A^-1 / Q / G / H products and none of their barriers.
// Per-segment scratch (doubles): the R_pp blocks -- W (coupling to the next inner vertex,
// then G = S^-1 E of the block solve) and L (diagonal block) -- and the powers of T.
struct Seg {
    static constexpr int kW = 0, kL = 16, kPow = 32, kX = 44, kSize = 56;  // kX: refinement's saved x (12)
};
// kPow: (1/T)^0..(1/T)^9 (A^-1's and H's negative powers) then T (H's one positive power)
constexpr int kNPow = 11;
__device__ __forceinline__ double seg_pow(const double* pw, int e) { return e > 0 ? pw[10] : pw[-e]; }  // T^e, e in [-9, 1]
__device__ __forceinline__ double hess(const double* kc, const double* pw, int r, int c) {
    return kc[kCH + r * 10 + c] * seg_pow(pw, (r % 5) + (c % 5) - 7);
}
// Per track, besides the segment scratch: (M+1) x 5 x 3 vertex values, (M+1) x 4 x 3
// right-hand sides, M segment times and the block solve's lane exchange (kXch, in LDS).
constexpr int kXch = 144;
__host__ __device__ constexpr size_t vertex_doubles(int M) { return (size_t)(M + 1) * 27 + (size_t)M + kXch; }
// Tracks with up to this many segments keep the segment scratch in LDS (~114 KB at 40).
constexpr int kMaxLdsSeg = 40;

// The constraint policy of solve_track: which derivatives of which vertices are prescribed
// besides the positions (the reference's Vertex::addConstraint, src/vertex.cpp:30-60).
//   NoPins        generateTrajectory's set: the start vertex {v0, a0, 0, 0}, the end vertex at
//                 rest, derivatives 1..4 of every inner vertex free.  solve_track compiles to
//                 the code it was before the policy existed.
//   VertexPins    (minsnap_constrained.hip) the caller's: all four derivatives of the two end
//                 vertices, and any subset of an inner vertex's.  mask: one byte per vertex
//                 (LDS), bit k-1 = derivative k is fixed, 0xF at the two ends; val: 12 doubles
//                 per vertex, (k-1) * 3 + d, read only where the bit is set.
// A fixed derivative of an inner vertex stays inside the 4 x 4 block system as a unit row and
// column (build_blocks) whose right-hand side is the value; the rows it coupled to take
// -R[row][fixed] * value into theirs (rhs_entry), as they do for the end vertices' values.
struct NoPins {
    static constexpr bool kOn = false;
};
struct VertexPins {
    static constexpr bool kOn = true;
    const uint8_t* mask;
    const double* val;
    __device__ __forceinline__ bool fixed(int v, int k) const { return (mask[v] >> (k - 1)) & 1; }
    __device__ __forceinline__ double value(int v, int k, int d) const { return val[((size_t)v * 4 + (k - 1)) * 3 + d]; }
};

// The min-snap solve of one track by one workgroup of BLOCK threads (every thread calls
// it; it contains barriers).  kc: the constants (LDS).  P: W x 3 waypoints; v0/a0: the start vertex's velocity and
// acceleration (NULL = 0); times_in: caller segment times (NULL = Nfabian).  scr: M x
// Seg::kSize, dv/rhs/Tm/xch: vertex_doubles(M) (LDS).  pins: the constraint policy (with
// VertexPins v0 / a0 are not read).  *s_err must be 0 and visible to every thread on entry.
// Writes T_out (M, may be NULL) and C_out (M x 3 x 10, increasing powers).  Returns 0, -2 (a segment time <= 0: the reference's
// CHECK_GT(segment_time, 0), impl :297) or -3 (R_pp not SPD).
template <int BLOCK, bool SCR_LDS, class PINS = NoPins>
__device__ __forceinline__ int solve_track(const double* __restrict__ kc, const double* __restrict__ P, int M, double vmax, double amax,
                                           const double* v0, const double* a0, const double* times_in,
                                           double* scr, double* dv, double* rhs, double* Tm, double* xch,
                                           int* s_err, double* T_out, double* C_out, bool refine,
                                           const PINS& pins = PINS()) {
    const int tid = threadIdx.x;
    // ---- phase 1: segment times, powers of T, fixed vertex values ---------------
    // (one barrier: every thread of a segment's powers takes its time itself -- the
    // caller's, or Nfabian of the same two waypoints, the same arithmetic each time)
    for (int e = tid; e < M * kNPow; e += BLOCK) {  // (1/T)^k, k = 0..9, and T
        const int i = e / kNPow, k = e % kNPow;
        const double T = times_in ? times_in[i] : nfabian(P + 3 * i, P + 3 * (i + 1), vmax, amax);
        if (k == 0) {
            Tm[i] = T;
            if (T_out) T_out[i] = T;
            if (!(T > 0)) atomicOr(s_err, 1);  // CHECK_GT(segment_time, 0)  impl :297
        }
        // 1/T: the hardware reciprocal refined by two Newton steps (~1e-16; a division
        // would cost ~10 dependent instructions)
        double it = __builtin_amdgcn_rcp(T);
        it = fma(it, fma(-T, it, 1.0), it);
        it = fma(it, fma(-T, it, 1.0), it);
        double p = k == 10 ? T : 1.0;
        for (int q = 0; q < k && k < 10; ++q) p = p * it;
        scr[(size_t)i * Seg::kSize + Seg::kPow + k] = p;
    }
    // start vertex {p0, v0, a0, 0, 0}, inner {p}, end {p, 0, 0, 0, 0}: makeStartOrEnd
    // (src/vertex.cpp:146-170) and trajectory_generator.cpp:28-50
    for (int e = tid; e < (M + 1) * 15; e += BLOCK) {
        const int v = e / 15, k = (e % 15) / 3, d = e % 3;
        double val = 0.0;  // free values are overwritten by the solve
        if (k == 0) val = P[3 * v + d];
        else if constexpr (PINS::kOn) val = pins.fixed(v, k) ? pins.value(v, k, d) : 0.0;  // (a free slot may hold NaN)
        else if (v == 0 && k == 1) val = v0 ? v0[d] : 0.0;
        else if (v == 0 && k == 2) val = a0 ? a0[d] : 0.0;
        dv[e] = val;
    }
    block_sync<SCR_LDS>();
    EPP_TL(1);
    if (*s_err) return -2;
    // ---- phase 2: block-tridiagonal system over the inner vertices ----------------
    // free variable (v, p): vertex v in 1..M-1, derivative p+1.  Diagonal block D_v is
    // kept in the L slot of segment v-1, the coupling E_v (v -> v+1) in the W slot.
    // Segment i's H (closed form, hess) couples vertex i (rows 0..4) and i+1 (rows 5..9).
    const int nin = M - 1;
    auto build_blocks = [&]() {
        for (int e = tid; e < nin * 16; e += BLOCK) {
            const int v = 1 + e / 16, p = (e % 16) / 4, q = e % 4;
            const double* pm = scr + (size_t)(v - 1) * Seg::kSize + Seg::kPow;
            const double* pp = scr + (size_t)v * Seg::kSize + Seg::kPow;
            if constexpr (PINS::kOn) {
                // a fixed (v, p+1): unit row and column of D_v, zero row of E_v; a fixed
                // (v+1, q+1): zero column of E_v
                const bool fd = pins.fixed(v, p + 1) | pins.fixed(v, q + 1);
                const bool fe = v >= nin || (pins.fixed(v, p + 1) | pins.fixed(v + 1, q + 1));
                scr[(size_t)(v - 1) * Seg::kSize + Seg::kL + p * 4 + q] =
                    fd ? (p == q ? 1.0 : 0.0) : hess(kc, pm, 6 + p, 6 + q) + hess(kc, pp, 1 + p, 1 + q);
                scr[(size_t)(v - 1) * Seg::kSize + Seg::kW + p * 4 + q] = fe ? 0.0 : hess(kc, pp, 1 + p, 6 + q);
                continue;
            }
            scr[(size_t)(v - 1) * Seg::kSize + Seg::kL + p * 4 + q] = hess(kc, pm, 6 + p, 6 + q) + hess(kc, pp, 1 + p, 1 + q);
            scr[(size_t)(v - 1) * Seg::kSize + Seg::kW + p * 4 + q] = (v < nin) ? hess(kc, pp, 1 + p, 6 + q) : 0.0;
        }
    };
    // b = -R_pf d_f, entry (v, p+1, d).  The two position columns of a segment enter as one
    // difference: H x u = 0 for u = e_0 + e_5 (moving both ends' positions together moves the
    // polynomial without changing its snap), so H[r][0] p_a + H[r][5] p_b = H[r][0] (p_a - p_b)
    // -- the same value without the cancellation of two large terms when the positions are
    // large next to their difference (hess(., 5) := -hess(., 0)).
    // (VertexPins: "fixed" is the mask's word, the two end vertices included; the row of a
    // fixed (v, p+1) is the unit row, its entry the value itself, which dv holds)
    auto is_fixed = [&](int vv, int k) -> bool {
        if constexpr (PINS::kOn) return pins.fixed(vv, k);
        else return vv == 0 || vv == M;
    };
    auto rhs_entry = [&](int v, int p, int d) -> double {
        if constexpr (PINS::kOn) {
            if (pins.fixed(v, p + 1)) return dv[(v * HALF + 1 + p) * 3 + d];
        }
        double s = 0.0;
        // segment v-1: rows 0..4 = vertex v-1, rows 5..9 = vertex v; row of (v,p+1) = 6+p
        {
            const double* pw = scr + (size_t)(v - 1) * Seg::kSize + Seg::kPow;
            s = hess(kc, pw, 6 + p, 0) * (dv[((v - 1) * HALF) * 3 + d] - dv[(v * HALF) * 3 + d]);
            for (int r = 1; r < N; ++r) {
                const int vv = (r < HALF) ? v - 1 : v, k = r % HALF;
                if (k != 0 && is_fixed(vv, k)) s = s + hess(kc, pw, 6 + p, r) * dv[(vv * HALF + k) * 3 + d];
            }
        }
        // segment v: rows 0..4 = vertex v (row of (v,p+1) = 1+p), rows 5..9 = vertex v+1
        {
            const double* pw = scr + (size_t)v * Seg::kSize + Seg::kPow;
            s = s + hess(kc, pw, 1 + p, 0) * (dv[(v * HALF) * 3 + d] - dv[((v + 1) * HALF) * 3 + d]);
            for (int r = 1; r < N; ++r) {
                const int vv = (r < HALF) ? v : v + 1, k = r % HALF;
                if (k != 0 && is_fixed(vv, k)) s = s + hess(kc, pw, 1 + p, r) * dv[(vv * HALF + k) * 3 + d];
            }
        }
        return -s;
    };
    build_blocks();
    for (int e = tid; e < nin * 12; e += BLOCK) {
        const int v = 1 + e / 12, p = (e % 12) / 3, d = e % 3;
        rhs[(v * 4 + p) * 3 + d] = rhs_entry(v, p, d);
    }
    block_sync<SCR_LDS>();
    EPP_TL(5);
    EPP_TLC(14);
    // ---- phase 3: block-tridiagonal solve (twisted block Thomas, lanes over the block entries)
    // Inner vertices v = 1..nin, diagonal blocks D_v, couplings E_v (v -> v+1), right-hand
    // sides b_v (3 columns).  Two eliminations run at once and meet at m = (nin+1)/2:
    //   top    (v = 1..m-1): S_1 = D_1, y_1 = b_1;  G_v = S_v^-1 E_v, g_v = S_v^-1 y_v;
    //                        S_{v+1} = D_{v+1} - E_v^T G_v,  y_{v+1} = b_{v+1} - E_v^T g_v
    //   bottom (v = nin..m+1): T_nin = D_nin, z_nin = b_nin;  H_v = T_v^-1 E_{v-1}^T,
    //                        h_v = T_v^-1 z_v;  T_{v-1} = D_{v-1} - E_{v-1} H_v, z likewise
    //   middle: x_m = (D_m - E_{m-1}^T G_{m-1} - E_m H_{m+1})^-1 (b_m - ...) -- the full Schur
    //           complement of vertex m: the top's S_m minus the bottom's correction
    //   back:   x_v = g_v - G_v x_{v+1} (v = m-1..1) and x_v = h_v - H_v x_{v-1} (v = m+1..nin),
    //           both directions at once.
    // The same elimination as one sweep from the top, in about half the dependent steps
    // (11 inner vertices: 5 + 1 + 5 instead of 11 + 11).  Lanes 0..27 run the top, lanes
    // 32..59 the bottom (the same instructions: the bottom reads its coupling transposed).
    // In a group, lane L owns one entry: L < 16 the 4x4 block entry (L>>2, L&3), 16..27
    // the 4x3 right-hand-side entry ((L-16)/3, (L-16)%3).  A step is two LDS-exchanged
    // stages: (1) adj(S) (one cofactor per lane); (2) every lane reads all of adj(S) and
    // forms the column t = adj(S) X of its own right-hand side X (coupling column for block
    // lanes, y column for rhs lanes) while det(S) and its reciprocal are computed beside
    // it; its entry of [G g] = t / det (kept for the back substitution) and of
    // [S' y'] = [D b] - E^T t / det (the next step's S, exchanged) follow without another
    // exchange.  S^-1 = adj(S) / det(S): no pivots or square roots; the Schur complements
    // of an SPD R_pp are SPD (det > 0), and the explicit inverse is within ~cond(S) ulp of
    // a factorisation's answer (parity target 1e-6).  Every value a step needs that does
    // not depend on the chain (the coupling, the next D / b entry) is loaded at its start.
    // G_v / H_v are kept in segment v-1's L slot (D_v is consumed by then), g_v / h_v in
    // rhs[v].  xch: per group (base 48 g) S|y [0,28), adj(S) [28,44); x buffers
    // [96 + 24 g, +24).
    auto block_solve = [&]() {
    if (tid < kWave && nin > 0) {
        const int L = tid & 31, grp = tid >> 5;
        const bool mat = L < 16, act = L < 28;
        const int row = mat ? (L >> 2) : (L - 16) / 3;  // block row (S, G) or rhs row (y, g)
        const int col = mat ? (L & 3) : (L - 16) % 3;
        const int ycol = mat ? 0 : col;                   // (block lanes read a dummy y column)
        const bool diag = mat && (L % 5) == 0;            // S[i][i]: must stay > 0 (SPD)
        const int m = (nin + 1) / 2;
        const int nstep = nin - m;                        // the bottom's steps (the top's: m - 1 <= nstep)
        const int gsteps = grp == 0 ? m - 1 : nin - m;
        double* xg = xch + 48 * grp;
        const int vs = grp == 0 ? 1 : nin;
        double cur = act ? (mat ? scr[(size_t)(vs - 1) * Seg::kSize + Seg::kL + L] : rhs[(size_t)vs * 12 + (L - 16)])
                         : 1.0;  // this lane's S / y entry
        if (act) xg[L] = cur;
        bool ok = !act || !diag || cur > 0.0;
        // the cofactor this lane computes: adj(S)[ar][ac] = (-1)^(ar+ac) det(S minus row ac, col ar)
        const int ar = (L >> 2) & 3, ac = L & 3;
        const int r0 = ac == 0 ? 1 : 0, r1 = ac <= 1 ? 2 : 1, r2 = ac <= 2 ? 3 : 2;
        const int c0 = ar == 0 ? 1 : 0, c1 = ar <= 1 ? 2 : 1, c2 = ar <= 2 ? 3 : 2;
        const double sgn = ((ar + ac) & 1) ? -1.0 : 1.0;
        // one elimination step on S|y in xg with coupling rows Ep (E^T row `row`) and
        // columns Ec (block lanes' X); returns t (4) and 1/det; ok updated
        auto step_core = [&](const double (&Ec)[4], double (&t)[4], double& id, bool live) {
            const double a = xg[r0 * 4 + c0], b = xg[r0 * 4 + c1], c = xg[r0 * 4 + c2];
            const double d = xg[r1 * 4 + c0], e = xg[r1 * 4 + c1], f = xg[r1 * 4 + c2];
            const double g = xg[r2 * 4 + c0], h = xg[r2 * 4 + c1], i = xg[r2 * 4 + c2];
            double s0[4], yc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s0[k] = xg[k];
                yc[k] = xg[16 + k * 3 + ycol];
            }
            const double m0 = fma(e, i, -(f * h)), m1 = fma(d, i, -(f * g)), m2 = fma(d, h, -(e * g));
            const double cof = sgn * fma(c, m2, fma(a, m0, -(b * m1)));
            if (mat && live) xg[28 + L] = cof;
            wave_sync_lds();
            double adj[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) adj[k] = xg[28 + k];
            const double det = fma(s0[0], adj[0], s0[1] * adj[4]) + fma(s0[2], adj[8], s0[3] * adj[12]);
            id = __builtin_amdgcn_rcp(det);  // refined by two Newton steps
            id = fma(id, fma(-det, id, 1.0), id);
            id = fma(id, fma(-det, id, 1.0), id);
            ok = ok && (!live || det > 0.0);
            double X[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) X[k] = mat ? Ec[k] : yc[k];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                t[k] = fma(adj[4 * k], X[0], adj[4 * k + 1] * X[1]) + fma(adj[4 * k + 2], X[2], adj[4 * k + 3] * X[3]);
        };
        wave_sync_lds();
        for (int s = 0; s < nstep; ++s) {
            EPP_TLI(1 + s);
            const bool live = s < gsteps;
            const int v = grp == 0 ? 1 + s : nin - s;
            const int vn = grp == 0 ? v + 1 : v - 1;  // the next vertex of this sweep
            // coupling: top E_v (segment v-1's W slot, E[k][q] at 4k + q), bottom E_{v-1}
            // transposed (segment v-2's W slot); E^T row `row`, and column `col`
            const double* Eb = scr + (size_t)(grp == 0 ? v - 1 : max(v - 2, 0)) * Seg::kSize + Seg::kW;
            double Ep[4], Ec[4], nxt = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Ep[k] = grp == 0 ? Eb[k * 4 + (row & 3)] : Eb[(row & 3) * 4 + k];
                Ec[k] = grp == 0 ? Eb[k * 4 + (col & 3)] : Eb[(col & 3) * 4 + k];
            }
            if (live && act) nxt = mat ? scr[(size_t)(vn - 1) * Seg::kSize + Seg::kL + L] : rhs[(size_t)vn * 12 + (L - 16)];
            double t[4], id;
            step_core(Ec, t, id, live);
            const double tr = row == 0 ? t[0] : row == 1 ? t[1] : row == 2 ? t[2] : t[3];
            const double et = fma(Ep[0], t[0], Ep[1] * t[1]) + fma(Ep[2], t[2], Ep[3] * t[3]);
            if (live && act) {
                if (mat) scr[(size_t)(v - 1) * Seg::kSize + Seg::kL + L] = tr * id;  // G_v / H_v
                else rhs[(size_t)v * 12 + (L - 16)] = tr * id;                       // g_v / h_v
                const double corr = et * id;
                cur = nxt - corr;  // [S' y'] = [D b] - E^T t / det
                // (the bottom's last step publishes its correction instead: the middle block
                // is the top's S_m minus it)
                xg[L] = (grp == 1 && s == nstep - 1) ? corr : cur;
                ok = ok && (!diag || cur > 0.0);
            }
            wave_sync_lds();
        }
        // middle: the top's S_m | y_m minus the bottom's last correction
        if (grp == 0 && act) {
            cur = cur - (nstep > 0 ? xch[48 + L] : 0.0);
            xg[L] = cur;
            ok = ok && (!diag || cur > 0.0);
        }
        wave_sync_lds();
        {
            const double Ec0[4] = {0.0, 0.0, 0.0, 0.0};
            double t[4], id;
            step_core(Ec0, t, id, grp == 0);
            const double tr = row == 0 ? t[0] : row == 1 ? t[1] : row == 2 ? t[2] : t[3];
            if (grp == 0 && act && !mat) {  // x_m = (middle block)^-1 (middle rhs)
                const double x = tr * id;
                rhs[(size_t)m * 12 + (L - 16)] = x;
                // derivatives 1..4 of vertex m (a fixed one keeps its given value in dv, not
                // the unit row's answer, which is the value to rounding)
                if constexpr (PINS::kOn) {
                    if (!pins.fixed(m, row + 1)) dv[((size_t)m * HALF + 1) * 3 + (L - 16)] = x;
                } else {
                    dv[((size_t)m * HALF + 1) * 3 + (L - 16)] = x;
                }
                xch[96 + (L - 16)] = x;
                xch[96 + 24 + (L - 16)] = x;
            }
        }
        // (the G/g stores, LDS or, for long tracks, global scratch: a workgroup-scope fence
        // makes the latter visible to the wave's own later loads)
        if (!SCR_LDS) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        wave_sync_lds();
        if (__ballot(!ok) == 0ull) {  // wave-uniform
            EPP_TLI(32);
            // lanes 0..11 of each group: x_v entry (p, d) = (L/3, L%3); the next step's G / H
            // row and g / h entry are loaded before this step's exchange completes
            const int p = (L / 3) & 3, d = L % 3;
            const int Lr = L < 12 ? L : 0;
            const int bsteps = grp == 0 ? m - 1 : nin - m;
            double* xb = xch + 96 + 24 * grp;
            int buf = 0;
            double Gr[4] = {0.0, 0.0, 0.0, 0.0}, gx = 0.0;
            auto load_step = [&](int v, double (&G)[4], double& gg) {
                const double* Gp = scr + (size_t)(v - 1) * Seg::kSize + Seg::kL + p * 4;
#pragma unroll
                for (int k = 0; k < 4; ++k) G[k] = Gp[k];
                gg = rhs[(size_t)v * 12 + Lr];
            };
            if (bsteps > 0) load_step(grp == 0 ? m - 1 : m + 1, Gr, gx);
            for (int s = 0; s < nstep; ++s) {
                EPP_TLI(33 + s);
                const bool live = s < bsteps;
                const int v = grp == 0 ? m - 1 - s : m + 1 + s;
                double Gn[4] = {0.0, 0.0, 0.0, 0.0}, gn = 0.0;
                if (s + 1 < bsteps) load_step(grp == 0 ? v - 1 : v + 1, Gn, gn);
                const double* xn = xb + buf * 12;
                const double x = gx - (fma(Gr[0], xn[d], Gr[1] * xn[3 + d]) + fma(Gr[2], xn[6 + d], Gr[3] * xn[9 + d]));
                if (live && L < 12) {
                    xb[(buf ^ 1) * 12 + L] = x;
                    // derivatives 1..4 of vertex v
                    if constexpr (PINS::kOn) {
                        if (!pins.fixed(v, p + 1)) dv[((size_t)v * HALF + 1) * 3 + L] = x;
                    } else {
                        dv[((size_t)v * HALF + 1) * 3 + L] = x;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) Gr[k] = Gn[k];
                gx = gn;
                buf ^= 1;
                wave_sync_lds();
            }
        } else if (tid == 0) {
            *s_err = 1;
        }
        EPP_TLI(63);
    }
    };
    block_solve();
    block_sync<SCR_LDS>();
    EPP_TL(6);
    EPP_TLC(15);
    if (*s_err) return -3;
    // ---- one step of iterative refinement (refine): r = b - R_pp x (the closed-form blocks
    // again: the solve consumed the L slots), R_pp dx = r by the same elimination, x += dx.
    // The elimination's rounding is amplified by R_pp's condition (up to ~1e12 next to very
    // short segments); one step brings the solution to the accuracy of the data.
    if (refine && nin > 0) {
        for (int e = tid; e < nin * 12; e += BLOCK) {
            const int v = 1 + e / 12, p = (e % 12) / 3, d = e % 3;
            const double* pm = scr + (size_t)(v - 1) * Seg::kSize + Seg::kPow;  // segment v-1
            const double* pp = scr + (size_t)v * Seg::kSize + Seg::kPow;        // segment v
            double r = rhs_entry(v, p, d);
            if constexpr (PINS::kOn) {
                // the masked blocks: a fixed row's residual is value - dv = 0; a free row's
                // sum leaves the fixed columns out (rhs_entry took them)
                if (pins.fixed(v, p + 1)) {
                    r = 0.0;
                } else {
                    for (int q = 0; q < 4; ++q) {
                        if (!pins.fixed(v, q + 1))
                            r = r - (hess(kc, pm, 6 + p, 6 + q) + hess(kc, pp, 1 + p, 1 + q)) * dv[(v * HALF + 1 + q) * 3 + d];
                        if (v < nin && !pins.fixed(v + 1, q + 1))
                            r = r - hess(kc, pp, 1 + p, 6 + q) * dv[((v + 1) * HALF + 1 + q) * 3 + d];
                        if (v > 1 && !pins.fixed(v - 1, q + 1))
                            r = r - hess(kc, pm, 1 + q, 6 + p) * dv[((v - 1) * HALF + 1 + q) * 3 + d];
                    }
                }
                rhs[(v * 4 + p) * 3 + d] = r;
                continue;
            }
            for (int q = 0; q < 4; ++q) {
                r = r - (hess(kc, pm, 6 + p, 6 + q) + hess(kc, pp, 1 + p, 1 + q)) * dv[(v * HALF + 1 + q) * 3 + d];
                if (v < nin) r = r - hess(kc, pp, 1 + p, 6 + q) * dv[((v + 1) * HALF + 1 + q) * 3 + d];
                if (v > 1) r = r - hess(kc, pm, 1 + q, 6 + p) * dv[((v - 1) * HALF + 1 + q) * 3 + d];
            }
            rhs[(v * 4 + p) * 3 + d] = r;
        }
        block_sync<SCR_LDS>();
        for (int e = tid; e < nin * 12; e += BLOCK) {  // x kept in the segments' X slots
            const int v = 1 + e / 12, p = (e % 12) / 3, d = e % 3;
            scr[(size_t)(v - 1) * Seg::kSize + Seg::kX + p * 3 + d] = dv[(v * HALF + 1 + p) * 3 + d];
        }
        build_blocks();
        block_sync<SCR_LDS>();
        block_solve();
        block_sync<SCR_LDS>();
        if (*s_err) return -3;
        for (int e = tid; e < nin * 12; e += BLOCK) {
            const int v = 1 + e / 12, p = (e % 12) / 3, d = e % 3;
            if constexpr (PINS::kOn) {
                if (pins.fixed(v, p + 1)) continue;  // (the second solve left the given value in dv, too)
            }
            double& x = dv[(v * HALF + 1 + p) * 3 + d];
            x = scr[(size_t)(v - 1) * Seg::kSize + Seg::kX + p * 3 + d] + x;
        }
        block_sync<SCR_LDS>();
    }
    // ---- phase 4: p_i = A_i^-1 [d_i ; d_{i+1}] -------------------------------------
    for (int e = tid; e < M * 30; e += BLOCK) {
        const int i = e / 30, d = (e % 30) / 10, r = e % 10;
        const double* ipow = scr + (size_t)i * Seg::kSize + Seg::kPow;
        const double* d0 = dv + (size_t)i * HALF * 3 + d;  // vertex i's values, then vertex i+1's
        double s;
        if (r < HALF) {  // rows 0..4 of A^-1: diag(1 / r!)
            s = kc[kCF + r] * d0[3 * r];
        } else {  // rows 5..9: [K | B5^-1] row rr, column c scaled by (1/T)^(rr + 5 - c % 5)
            // (the two positions as one difference: K[rr][0] = -B5^-1[rr][0], A^-1 maps equal
            // end positions to a constant polynomial)
            const int rr = r - HALF;
            s = kc[kCK + rr * HALF] * ipow[rr + HALF] * (d0[0] - d0[3 * HALF]);
#pragma unroll
            for (int k = 1; k < N; ++k) {
                if (k == HALF) continue;
                const double a = (k < HALF ? kc[kCK + rr * HALF + k] : kc[kCB5 + rr * HALF + k - HALF]) *
                                 ipow[rr + HALF - k % HALF];
                s = s + a * d0[3 * k];
            }
        }
        C_out[((size_t)i * 3 + d) * N + r] = s;
    }
    return 0;
}

}  // namespace
}  // namespace epp
