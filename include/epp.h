/*
 * epp.h — C ABI of the MI355X-native Efficient-Path-Planner hot path.
 *
 * Plain pointers and sizes only; no torch / Eigen / OMPL types.  Every compute
 * entry point is stream-ordered on the hipStream_t passed as `void* stream`
 * (NULL = the null stream) and takes DEVICE pointers for bulk data (pinned host memory
 * from hipHostMalloc also works: the kernels then read / write it over the bus, which
 * the host-array paths use for small batches).  All
 * functions return an epp_status (0 = ok, < 0 = error); the message of the last
 * error on the calling thread is available from epp_last_error().
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference repository root):
 *
 *   epp_world_create / epp_world_update
 *       World::addGate / addObstacle / updateGatePosition / resetWorld
 *       (include/World.h:27-56, src/World.cpp:13-78) — OBB table + AABB index
 *       (the Boost rtree `index`, include/World.h:109) uploaded to HBM.
 *   epp_check_states
 *       StateValidator::isValid (include/StateValidator.h:31, src/StateValidator.cpp:7-13)
 *       -> World::checkPointValidity(p, canPassGate) (src/World.cpp:80-104), batched.
 *   epp_check_states_mindist
 *       World::checkPointValidity(p, minDistance) (src/World.cpp:106-128) as used by
 *       PathPlanner::checkTrajectoryValidity (src/PathPlanner.cpp:267-280).
 *   epp_check_motions
 *       MotionValidator::checkMotion (include/MotionValidator.h:26, src/MotionValidator.cpp:8-17)
 *       -> World::checkRayValid (src/World.cpp:130-162), batched; mode 1 adds the
 *       32-step discretised check of BASELINE config 3.
 *   epp_minsnap_batch / epp_sample_count / epp_sample_batch
 *       poly_traj::generateTrajectory (external/poly_traj/include/poly_traj/trajectory_generator.h:20,
 *       external/poly_traj/src/trajectory_generator.cpp:12-100), batched over tracks.
 *   epp_traj_check_batch
 *       PathPlanner::checkTrajectoryValidity (src/PathPlanner.cpp:267-280) of every fitted
 *       track, from its coefficients: the first failing row per track.
 *   epp_traj_sweep_batch
 *       World::checkRayValid (src/World.cpp:130-162) on the chords between consecutive rows
 *       of every fitted track: the first failing chord per track.
 *   epp_states_clearance / epp_traj_clearance_batch
 *       no reference counterpart: the Euclidean distance to the nearest collision OBB, per
 *       state and as the closest approach of every fitted track's rows.
 *   epp_motions_clearance / epp_traj_chord_clearance_batch
 *       no reference counterpart: the Euclidean distance between a straight edge and the
 *       nearest collision OBB, per edge and as the closest approach of the chords between the
 *       rows of every fitted track.
 *   epp_motions_first_hit / epp_traj_first_hit_batch
 *       what MotionValidator::checkMotion(s1, s2, lastValid) (src/MotionValidator.cpp:19-22, a
 *       stub there) needs: where along a straight edge World::checkRayValid first fails and
 *       against which OBB, per edge and for the first failing chord of every fitted track.
 *   epp_gates_crossed / epp_traj_gate_pass_batch
 *       OnlineTrajGenerator::checkGatePassed (src/OnlineTrajGenerator.cpp:228-256), per edge
 *       and gate, and as the ordered passage of every fitted track's chords with split times.
 *   epp_sample_derivative_batch
 *       Trajectory::evaluateRange(t_start, t_end, dt, derivative_order, ...)
 *       (external/poly_traj/src/trajectory.cpp:81-141) for any derivative, batched over tracks.
 *   epp_thrust_rates / epp_traj_thrust_rates_batch
 *       no reference counterpart: the thrust, the roll / pitch body rate and the tilt a
 *       quadrotor needs at a sample, and their extremes over every fitted track's rows.
 *   epp_traj_thrust_grid_batch / epp_traj_scale_to_thrust_limits
 *       Trajectory::scaleSegmentTimesToMeetConstraints (external/poly_traj/src/trajectory.cpp:
 *       385-429) extended from |v| and |a| to thrust, body-rate and tilt limits: the extremes
 *       over the peak search's grid points at a scale, and the search for the scale.
 *   epp_traj_snap_cost / epp_minsnap_time_gradient / epp_minsnap_optimize_times
 *       PolynomialOptimization::computeCost (impl/polynomial_optimization_linear_impl.h:123-140),
 *       getCostAndGradientMellinger (impl/polynomial_optimization_nonlinear_impl.h:286-364, which
 *       the reference ships commented out: its optimiser is NLopt) and a projected descent over
 *       the segment times at constant total time in its place.
 */
#ifndef EPP_H_
#define EPP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t epp_status;
#define EPP_OK 0
#define EPP_ERR_INVALID_ARGUMENT (-1) /* std::invalid_argument in the reference */
#define EPP_ERR_RUNTIME (-2)          /* std::runtime_error in the reference */
#define EPP_ERR_HIP (-3)              /* HIP runtime error */
#define EPP_ERR_UNSUPPORTED (-4)      /* rotation other than about z (src/Object.cpp:38-47) */
#define EPP_ERR_CAPACITY (-5)         /* an output buffer was too small */
#define EPP_ERR_PEER (-6)             /* another rank of a collective reported a failure */
#define EPP_ERR_TIMEOUT (-7)          /* a collective did not complete within the communicator's timeout */

/* An oriented bounding box after the world build (reference class OBB,
 * include/OBB.h:19-57).  rot is the row-major rotation matrix; the reference only
 * produces rotations about z (src/Object.cpp:61-85) and so does this ABI. */
typedef struct epp_obb {
    double center[3];
    double half[3];
    double rot[9];
    int32_t filling; /* OBB::type == "filling" (else "collision") */
    int32_t is_gate; /* World key contains "gate": selects the gate inflate radius */
} epp_obb;

/* One OBB of a component's geometry (config `component_geometry.<comp>.<obb>`,
 * src/ConfigParserYAML.cpp:54-73): position relative to the component origin and
 * full size (the half size is size / 2). */
typedef struct epp_obb_desc {
    double pos[3];
    double size[3];
    int32_t filling; /* "filling" (1) or "collision" (0) */
    int32_t pad;
} epp_obb_desc;

typedef struct epp_world epp_world; /* opaque, bound to one device */

/* ---- runtime ---------------------------------------------------------------------- */
const char* epp_last_error(void);
const char* epp_version(void);
epp_status epp_device_count(int* count);
epp_status epp_set_device(int device);
/* The compute units of the current device (the number the persistent grids of the k_traj_*
 * kernels are sized by: at most 8 workgroups per compute unit). */
epp_status epp_device_cu_count(int* count);
epp_status epp_malloc(void** ptr, uint64_t bytes);
epp_status epp_free(void* ptr);
epp_status epp_memcpy_h2d(void* dst, const void* src, uint64_t bytes, void* stream);
epp_status epp_memcpy_d2h(void* dst, const void* src, uint64_t bytes, void* stream);
/* Stream-ordered copies that return without waiting (epp_memcpy_* above synchronise the
 * stream); the host side should be pinned (page-locked) memory and must stay
 * untouched until the stream is synchronised. */
epp_status epp_memcpy_h2d_async(void* dst, const void* src, uint64_t bytes, void* stream);
epp_status epp_memcpy_d2h_async(void* dst, const void* src, uint64_t bytes, void* stream);
epp_status epp_memset(void* dst, int value, uint64_t bytes, void* stream);
epp_status epp_stream_create(void** stream);
epp_status epp_stream_destroy(void* stream);
epp_status epp_stream_sync(void* stream);
epp_status epp_device_sync(void);
epp_status epp_event_create(void** event);
epp_status epp_event_destroy(void* event);
epp_status epp_event_record(void* event, void* stream);
epp_status epp_event_elapsed_ms(void* start, void* stop, float* ms);
/* Stream capture of stream-ordered epp_* calls into an instantiated HIP graph and its
 * replay (no counterpart in the reference: launch-overhead tool for batched callers,
 * e.g. bench.py's timed steps). */
epp_status epp_graph_begin(void* stream);
epp_status epp_graph_end(void* stream, void** exec);
epp_status epp_graph_launch(void* exec, void* stream);
epp_status epp_graph_destroy(void* exec);

/* ---- world ------------------------------------------------------------------------ */
/* World::addGate / World::addObstacle (src/World.cpp:13-55) via
 * Object::createFromDescription (src/Object.cpp:26-85), on the host.
 * gates: n_gates x 7 row-major (x, y, z, roll, pitch, yaw, type) — z is forced to 0
 * (src/PathPlanner.cpp:68); obstacles: n_obstacles x 6 (x, y, z, roll, pitch, yaw).
 * Gate type t uses gate_desc[gate_desc_off[t] .. gate_desc_off[t+1]).  Errors:
 * EPP_ERR_UNSUPPORTED for |roll| or |pitch| > 1e-6, EPP_ERR_RUNTIME for an object
 * centre z > 1e-6 or an unknown gate type, EPP_ERR_CAPACITY if out is too small
 * (*n_out then holds the required count). */
epp_status epp_build_obbs(const epp_obb_desc* gate_desc, const int32_t* gate_desc_off,
                          int32_t n_gate_types, const epp_obb_desc* obst_desc, int32_t n_obst_desc,
                          const double* gates, int32_t n_gates, const double* obstacles,
                          int32_t n_obstacles, epp_obb* out, int32_t capacity, int32_t* n_out);

/* Builds the AABB of every OBB (OBB::getAABB, src/OBB.cpp:93-123, inflated only for
 * "collision" OBBs by r_gate or r_obst) and a uniform cull grid over them, and
 * uploads both to the current device.  obbs is a HOST array. */
epp_status epp_world_create(const epp_obb* obbs, int32_t n_obbs, double r_gate, double r_obst,
                            epp_world** out);
/* Replaces the OBB set (gate-pose update = full rebuild, src/OnlineTrajGenerator.cpp:146).
 * Rebuilds the OBB records only, into the one of two pinned host slots that is not the
 * current version's (after the asynchronous small-query launches that read that slot
 * have finished; nothing else is waited for): small queries (<= 4096 states or 1024
 * edges on worlds of <= 256 OBBs) read those directly; the device index is rebuilt and
 * uploaded by the first call that needs it (or epp_world_build_index), after every kernel
 * that may read the old index, so an index error (e.g. too many distinct candidate
 * lists) is reported there.  Checks may run on other host threads meanwhile: each launch
 * uses the version of the index it finds (the one before or after the update, never a mix;
 * a rebuild waits until launches holding the old one are queued).  HIP graphs
 * that captured launches on this world must be re-captured afterwards, and only after
 * epp_world_build_index (launch shapes depend on the index; epp_world_generation
 * changes). */
epp_status epp_world_update(epp_world* w, const epp_obb* obbs, int32_t n_obbs);
/* Rebuilds and uploads the device index now if an update left it stale (synchronous;
 * not inside a stream capture). */
epp_status epp_world_build_index(const epp_world* w);
/* Number of versions of this world so far (create = 1, every update + 1). */
epp_status epp_world_generation(const epp_world* w, uint64_t* generation);
epp_status epp_world_destroy(epp_world* w);
epp_status epp_world_num_obbs(const epp_world* w, int32_t* n);
/* Host copy of the AABBs computed for the index (lo[3], hi[3] per OBB). */
epp_status epp_world_get_aabbs(const epp_world* w, double* lo_hi);

/* ---- collision checks (device pointers) ------------------------------------------- */
/* xyz: n x 3 f64 (AoS).  valid[i] = 1 if state i is collision free.  If compact_idx
 * is non-NULL, the indices of valid states are appended to it and *n_valid (device
 * int64, caller zeroes it) receives the count; the order of the compacted indices
 * is unspecified (wavefront order is preserved, inter-wavefront order is not). */
epp_status epp_check_states(const epp_world* w, const double* xyz, int64_t n, int32_t can_pass_gate,
                            uint8_t* valid, int32_t* compact_idx, int64_t* n_valid, void* stream);
epp_status epp_check_states_mindist(const epp_world* w, const double* xyz, int64_t n,
                                    double min_distance, uint8_t* valid, void* stream);
/* s1, s2: n x 3 f64.  mode 0 = analytic slab test (reference), 1 = discrete32:
 * points s1 + (s2 - s1) * (k/32), k = 1..32, each checked like epp_check_states. */
epp_status epp_check_motions(const epp_world* w, const double* s1, const double* s2, int64_t n,
                             int32_t can_pass_gate, int32_t mode, uint8_t* valid, void* stream);

/* ---- min-snap trajectory (device pointers) ---------------------------------------- */
/* Track k owns waypoints [wp_offsets[k], wp_offsets[k+1]) of wp (x,y,z f64) and
 * segments [wp_offsets[k]-k, wp_offsets[k+1]-k-1).  v0/a0: n_tracks x 3 (NULL = 0).
 * Outputs: seg_times (total segments), coeffs (total segments x 3 x 10, increasing
 * powers, the layout of mav_trajectory_generation::Polynomial).  status (n_tracks,
 * may be NULL): 0 ok, -1 fewer than 2 waypoints, -2 non-positive segment time,
 * -3 solver breakdown. */
epp_status epp_minsnap_batch(const double* wp, const int32_t* wp_offsets, int32_t n_tracks,
                             double v_max, double a_max, const double* v0, const double* a0,
                             double* seg_times, double* coeffs, int32_t* status, void* stream);
/* As epp_minsnap_batch with the caller's segment times instead of
 * estimateSegmentTimesNfabian: PolynomialOptimization<10>::setupFromVertices(vertices,
 * segment_times) (impl/polynomial_optimization_linear_impl.h:56-109), as the reference's
 * own tests call it (external/poly_traj/test/test_polynomial_optimization.cpp:765-769).
 * seg_times_in: total segments (device).  status -2 for a segment time <= 0. */
epp_status epp_minsnap_batch_times(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, const double* v0,
                                   const double* a0, const double* seg_times_in, double* coeffs, int32_t* status,
                                   void* stream);
/* As epp_minsnap_batch with the caller's constraints on the vertices instead of
 * generateTrajectory's fixed set: what the reference's library takes through
 * Vertex::addConstraint (external/poly_traj/src/vertex.cpp:30-60) and its generateTrajectory
 * never uses.  Per waypoint w of wp (all device):
 *   fixed_mask[w]   bit k-1 set: derivative k (1..4: velocity, acceleration, jerk, snap) is
 *                   fixed at w; a bit above bit 3 gives status -4
 *   fixed_val       12 doubles, the x, y, z of derivative k at (w*4 + (k-1))*3 + d
 * At the first and the last waypoint of a track all four derivatives are fixed
 * (Vertex::makeStartOrEnd, :146-170): the mask there is ignored and the four values are
 * read.  epp_minsnap_batch's fit is fixed_val = [v0, a0, 0, 0] at the start, zeros at the end
 * and mask 0 inside.  A slot whose bit is clear at an inner waypoint is never read (it may
 * hold NaN); a non-finite value in a slot that is used gives status -4.  A fixed derivative
 * is met exactly (the segments on both sides are built from the given value) and the rest
 * stay continuous; a waypoint with all four fixed splits the fit there.
 * seg_times_in (total segments, device; may be seg_times): the caller's segment times as in
 * epp_minsnap_batch_times, NULL: Nfabian times of the positions under v_max / a_max -- they
 * ignore the fixed values, as they ignore v0 in epp_minsnap_batch, so a track pinned to
 * speeds far from v_max wants the caller's times.  Outputs and status 0, -1, -2, -3 as
 * epp_minsnap_batch; a track with status -4 is left unwritten.
 * EPP_ERR_INVALID_ARGUMENT for a NULL fixed_mask or fixed_val with n_tracks > 0. */
epp_status epp_minsnap_batch_constrained(const double* wp, const int32_t* wp_offsets, int32_t n_tracks,
                                         double v_max, double a_max, const double* seg_times_in,
                                         const uint8_t* fixed_mask, const double* fixed_val, double* seg_times,
                                         double* coeffs, int32_t* status, void* stream);
/* Number of rows Trajectory::evaluateRange produces for every track (device int64 out). */
epp_status epp_sample_count(const double* seg_times, const int32_t* wp_offsets, int32_t n_tracks,
                            double dt, int64_t* row_counts, void* stream);
/* rows: written at row_offsets[k] (device int64, exclusive scan of the counts), each
 * row [x,vx,ax,y,vy,ay,z,vz,az,t+t0[k]]; t0 may be NULL (= 0). */
epp_status epp_sample_batch(const double* seg_times, const double* coeffs,
                            const int32_t* wp_offsets, int32_t n_tracks, double dt, const double* t0,
                            const int64_t* row_offsets, double* rows, void* stream);
/* Trajectory::computeMaxVelocityAndAcceleration (external/poly_traj/src/trajectory.cpp:344-361,
 * computeMinMaxMagnitude :191-227, over the per-segment magnitude extrema of
 * external/poly_traj/src/segment.cpp:83-185), batched over tracks in the layout of
 * epp_minsnap_batch.  peaks: n_tracks x 4 [v_peak, t_v, a_peak, t_a]: the maxima over the
 * whole track of the Euclidean norm (x, y, z) of the first and second derivative, and
 * where they occur, as time from the start of the track (the sum of the earlier segment
 * times plus the time in the segment; equal maxima report the earliest).  The extrema are
 * the segment ends and the roots of sum_d p_d^(k) p_d^(k+1), bracketed on 64 subintervals
 * per segment and bisected (not the reference's Jenkins-Traub roots of the convolved
 * polynomial): a subinterval holding two roots is not searched, so a bump of the magnitude
 * narrower than 1/64 of its segment can be missed.  status (n_tracks, may be NULL): 0 ok;
 * -1 fewer than one segment, a segment time <= 0 or non-finite input (the buffers of a
 * track that epp_minsnap_batch failed): its peaks are NaN. */
epp_status epp_traj_peaks(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                          int32_t n_tracks, double* peaks, int32_t* status, void* stream);
/* Trajectory::scaleSegmentTimesToMeetConstraints (external/poly_traj/src/trajectory.cpp:385-429)
 * per track, in place on seg_times and coeffs, the whole loop in one launch: at most 20
 * rounds of [peaks as epp_traj_peaks; vv = v_peak / v_max, av = a_peak / a_max; done when
 * both are <= 1 + 1e-3; else every segment time times s = max(1, vv, sqrt(av)) and every
 * polynomial scaled in time with 1 / s (Polynomial::scalePolynomialInTime,
 * external/poly_traj/src/polynomial.cpp:199-205)].  One factor for the whole track: the
 * path keeps its shape, x_new(s t) = x_old(t).  scale: n_tracks, the product of the
 * factors applied; a track within the limits comes back bit for bit with scale 1.0.
 * status (n_tracks, may be NULL): 0 within the limits; 1 still outside after 20 rounds;
 * -1 as epp_traj_peaks (the track is left untouched, scale 1.0).
 * EPP_ERR_INVALID_ARGUMENT for v_max <= 0 or a_max <= 0. */
epp_status epp_traj_scale_to_limits(double* seg_times, double* coeffs, const int32_t* wp_offsets,
                                    int32_t n_tracks, double v_max, double a_max, double* scale,
                                    int32_t* status, void* stream);
/* PathPlanner::checkTrajectoryValidity (src/PathPlanner.cpp:267-280) for every track of a
 * batch in the layout of epp_minsnap_batch, straight from the coefficients, in one launch
 * and without writing a row: first_invalid[k] (n_tracks, device int64) is the index of the
 * first row of Trajectory::evaluateRange(0, max_time, dt) (src/trajectory.cpp:81-141)
 * whose position fails World::checkPointValidity(p, min_distance) (src/World.cpp:106-128),
 * -1 if every row passes (a track without rows, e.g. of one waypoint or with the NaN times
 * of a failed fit, passes, as the reference's loop returns true).  first_time[k] (n_tracks,
 * device f64, may be NULL) is that row's time column as epp_sample_batch writes it with
 * t0 == NULL, -1.0 for a valid track.  The answers are those of epp_sample_count +
 * epp_sample_batch + epp_check_states_mindist on the rows' columns 0 / 3 / 6, bit for bit
 * (the same recurrence, Horner steps and predicates).  Stream-ordered, no host
 * synchronisation and no allocation; a stale world index is rebuilt first, as by
 * epp_check_states_mindist, so the call can be captured (epp_graph_begin) after
 * epp_world_build_index.  EPP_ERR_INVALID_ARGUMENT (before any device work) for a NULL
 * world, n_tracks < 0, dt <= 0 or not finite, or a NULL seg_times, coeffs, wp_offsets or
 * first_invalid with n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_traj_check_batch(const epp_world* w, const double* seg_times, const double* coeffs,
                                const int32_t* wp_offsets, int32_t n_tracks, double dt, double min_distance,
                                int64_t* first_invalid, double* first_time, void* stream);
/* The swept companion of epp_traj_check_batch (same layout, same contract): the rows only
 * say where the track is every dt, this call tests the straight chords between them.  With
 * p_0 .. p_{R-1} the positions of the rows of Trajectory::evaluateRange(0, max_time, dt) of
 * track k, chord j (0 <= j < R - 1) is p_j -> p_{j+1}, tested with World::checkRayValid(p_j,
 * p_{j+1}, can_pass_gate) (src/World.cpp:130-162; epp_check_motions mode 0).
 * first_invalid[k] (n_tracks, device int64) is the smallest j whose chord fails, -1 if none
 * does; first_time[k] (n_tracks, device f64, may be NULL) is the time column of row j as
 * epp_sample_batch writes it with t0 == NULL, -1.0 if none fails.  A track with fewer than
 * two rows (one waypoint, the NaN times of a failed fit) has no chord: -1 / -1.0.  The
 * answers are those of epp_sample_count + epp_sample_batch + epp_check_motions(s1 = rows j,
 * s2 = rows j + 1, columns 0 / 3 / 6, mode 0) per track, bit for bit (the same recurrence,
 * Horner steps and predicates; a zero-length chord takes the ray test's |d| < 1e-6 branches
 * as there).  Stream-ordered, no host synchronisation and no allocation; a stale world
 * index is rebuilt first, so the call can be captured after epp_world_build_index.
 * EPP_ERR_INVALID_ARGUMENT (before any device work) for a NULL world, n_tracks < 0, dt <= 0
 * or not finite, can_pass_gate not 0 or 1, or a NULL seg_times, coeffs, wp_offsets or
 * first_invalid with n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_traj_sweep_batch(const epp_world* w, const double* seg_times, const double* coeffs,
                                const int32_t* wp_offsets, int32_t n_tracks, double dt, int32_t can_pass_gate,
                                int64_t* first_invalid, double* first_time, void* stream);

/* ---- clearance: the Euclidean distance to the nearest collision OBB (device pointers) ---
 * For a point p and OBB i with filling == 0 (filling OBBs are skipped, as the minDistance
 * check skips them), every operation one IEEE fp64 multiply, add or subtract in this
 * association:
 *   dx = px - cx;  dy = py - cy;  dz = pz - cz
 *   lx = c*dx + s*dy;  ly = c*dy - s*dx              (c, s: the cos / sin of the OBB's yaw)
 *   ex = max(|lx| - hx, 0);  ey = max(|ly| - hy, 0);  ez = max(|dz| - hz, 0)   (not inflated)
 *   d2_i = (ex*ex + ey*ey) + ez*ez
 * d2(p) = min_i d2_i; the nearest OBB is the lowest index i, in the order given to
 * epp_world_create / epp_world_update, that attains it.  The distance is sqrt(d2), taken once
 * after the minimum: 0 inside or on a box.  No grid, no AABB prefilter and no inflate radius
 * take part, so a point far from everything has its exact distance.  A world without
 * collision OBBs gives +inf and OBB -1; a NaN d2_i never updates the minimum, so a
 * non-finite point gives +inf / -1 too.
 *
 * epp_states_clearance: dist[i] (n, device f64) and nearest[i] (n, device int32, may be
 * NULL) for each of the n states xyz (n x 3 f64).  Stream-ordered, no host synchronisation
 * and no allocation; a stale world index is rebuilt first, as by epp_check_states_mindist,
 * so the call can be captured (epp_graph_begin) after epp_world_build_index.
 * EPP_ERR_INVALID_ARGUMENT (before any device work) for a NULL world, n < 0, or a NULL xyz
 * or dist with n > 0; n == 0 launches nothing. */
epp_status epp_states_clearance(const epp_world* w, const double* xyz, int64_t n, double* dist, int32_t* nearest,
                                void* stream);
/* The closest approach of every track of a batch in the layout of epp_minsnap_batch, straight
 * from the coefficients, in one launch and without writing a row.  Over the positions of the
 * rows of Trajectory::evaluateRange(0, max_time, dt) of track k: clearance[k] (n_tracks,
 * device f64) is the square root of the minimum d2; row[k] (device int64, may be NULL) the
 * earliest row that attains it; time[k] (device f64, may be NULL) that row's time column as
 * epp_sample_batch writes it with t0 == NULL; nearest[k] (device int32, may be NULL) the
 * nearest OBB of that row.  A track without rows (one waypoint, the NaN times of a failed
 * fit) or a world without collision OBBs gives +inf, -1, -1.0, -1; rows with a non-finite
 * position are ignored.  The answers are those of epp_sample_count + epp_sample_batch +
 * epp_states_clearance on the rows' columns 0 / 3 / 6 followed by a per-track minimum that
 * prefers the earliest row, bit for bit (the same recurrence, Horner steps and d2, one
 * square root after an exact minimum).  Stream-ordered, no host synchronisation and no
 * allocation; a stale world index is rebuilt first, as by epp_check_states_mindist, so the
 * call can be captured (epp_graph_begin) after epp_world_build_index.
 * EPP_ERR_INVALID_ARGUMENT (before any device work) for a NULL world, n_tracks < 0, dt <= 0
 * or not finite, or a NULL seg_times, coeffs, wp_offsets or clearance with n_tracks > 0;
 * n_tracks == 0 launches nothing. */
epp_status epp_traj_clearance_batch(const epp_world* w, const double* seg_times, const double* coeffs,
                                    const int32_t* wp_offsets, int32_t n_tracks, double dt, double* clearance,
                                    int64_t* row, double* time, int32_t* nearest, void* stream);

/* ---- swept clearance: the Euclidean distance between a straight edge and the nearest
 * collision OBB (device pointers).  For the edge s -> e and OBB i with filling == 0, both
 * endpoints go into the box frame by the operations of the clearance above (a from s, b from
 * e; h the half sizes, not inflated) and d = b - a per axis.  Along the edge q(t) = a + t*d
 * per axis, and for a local point q
 *   F(q) = (ex*ex + ey*ey) + ez*ez,   e_k = max(|q_k| - h_k, 0)             (the d2 above)
 *   G(q) = (wx + wy) + wz,            w_k = e_k * (q_k < 0 ? -d_k : d_k)    (half of df/dt)
 * f(t) = F(q(t)) is convex and piecewise quadratic.  The candidates, in this order, taken into
 * a running minimum that starts at +inf on a strict <:
 *   1. t = 0:  f = F(a), the d2_i of the point s above, bit for bit
 *   2. t = 1:  f = F(b), the d2_i of the point e
 *   3. axes x, y, z, for each the face -h_k then +h_k:  t = (-+h_k - a_k) / d_k, kept iff
 *      0 < t < 1:  f = F(q(t)).  The bracket of G's zero: (tl, gl) starts at (0, G(a)) and
 *      (tr, gr) at (1, G(b)); a kept t with g = G(q(t)) < 0 and t > tl replaces (tl, gl), one
 *      with g >= 0 and t < tr replaces (tr, gr)
 *   4. iff G(a) < 0 < G(b):  t* = tl + (tr - tl) * ((-gl) / (gr - gl)),  f = F(q(t*))
 * d2_i is the smallest f and t_i the candidate that gave it; every operation is one IEEE fp64
 * multiply, add, subtract or divide in this association, nothing fused, every choice a select
 * on a compare (a NaN compares false).  d2(edge) = min_i d2_i over every OBB in the order given
 * to epp_world_create / epp_world_update on a strict <: the nearest OBB is the lowest index
 * that attains it, t_min its t_i, and the distance is sqrt(d2), taken once after the minimum:
 * 0 for an edge that touches or enters a box.  No grid, no AABB prefilter and no inflate
 * radius take part.  So d2(edge) <= min(d2(s), d2(e)) of the clearance above as doubles, and a
 * zero-length edge has exactly the distance and OBB of its point.  Against the exact minimum
 * of f the measured error of d2 is 5.1e-16 * max(1, L^2), L the largest coordinate difference
 * between an endpoint and the nearest box's centre.  A world without collision
 * OBBs gives +inf, t_min -1.0 and OBB -1, and so does an edge with a coordinate that is not
 * finite, which takes part in no minimum.
 *
 * epp_motions_clearance: dist[i] (n, device f64), t_min[i] (n, device f64, may be NULL) and
 * nearest[i] (n, device int32, may be NULL) for each of the n edges s1[i] -> s2[i] (n x 3 f64
 * each).  Stream-ordered, no host synchronisation and no allocation; a stale world index is
 * rebuilt first, as by epp_states_clearance, so the call can be captured (epp_graph_begin)
 * after epp_world_build_index.  EPP_ERR_INVALID_ARGUMENT (before any device work) for a NULL
 * world, n < 0, or a NULL s1, s2 or dist with n > 0; n == 0 launches nothing. */
epp_status epp_motions_clearance(const epp_world* w, const double* s1, const double* s2, int64_t n, double* dist,
                                 double* t_min, int32_t* nearest, void* stream);
/* The closest approach of the chords of every track of a batch in the layout of
 * epp_minsnap_batch, straight from the coefficients, in one launch and without writing a row.
 * Over the chords row j -> row j + 1 of the rows of Trajectory::evaluateRange(0, max_time, dt)
 * of track k: clearance[k] (n_tracks, device f64) is the square root of the minimum d2;
 * chord[k] (device int64, may be NULL) the earliest j that attains it; t[k] (device f64, may be
 * NULL) that chord's t_min; time[k] (device f64, may be NULL) = t_j + t * (t_j+1 - t_j) on the
 * time columns epp_sample_batch writes with t0 == NULL: one subtract, one multiply, one add,
 * unfused; nearest[k] (device int32, may be NULL) that chord's nearest OBB.  A track with
 * fewer than two rows (one waypoint, the NaN times of a failed fit) or a world without
 * collision OBBs gives +inf, -1, -1.0, -1.0, -1; a chord with a non-finite end is ignored.
 * The answers are those of epp_sample_count + epp_sample_batch + epp_motions_clearance(s1 =
 * rows j, s2 = rows j + 1, columns 0 / 3 / 6) followed by a per-track minimum that prefers the
 * earliest chord, bit for bit (the same recurrence, Horner steps and d2, one square root after
 * an exact minimum).  So clearance[k] <= epp_traj_clearance_batch's for every track with two
 * rows or more.  Stream-ordered, no host synchronisation and no allocation; a stale world
 * index is rebuilt first, so the call can be captured (epp_graph_begin) after
 * epp_world_build_index.  EPP_ERR_INVALID_ARGUMENT (before any device work) for a NULL world,
 * n_tracks < 0, dt <= 0 or not finite, or a NULL seg_times, coeffs, wp_offsets or clearance
 * with n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_traj_chord_clearance_batch(const epp_world* w, const double* seg_times, const double* coeffs,
                                          const int32_t* wp_offsets, int32_t n_tracks, double dt, double* clearance,
                                          int64_t* chord, double* t, double* time, int32_t* nearest, void* stream);

/* ---- first hit: where a straight edge is first blocked, and by which OBB (device pointers)
 * For the edge s -> e, can_pass_gate and OBB i with owner radius r (r_gate for a gate's OBB,
 * r_obst otherwise), the candidates are exactly the OBBs World::checkRayValid
 * (src/World.cpp:130-162) would test: OBB i takes part iff its stored inflated AABB overlaps
 * the edge's bounding box [min(s, e), max(s, e)], closed on both sides, and it is not a
 * filling OBB with can_pass_gate == 1.  On a candidate, OBB::checkCollisionWithRay
 * (src/OBB.cpp:10-61) is evaluated as by epp_check_motions (mode 0), every operation one IEEE
 * fp64 multiply, add, subtract or divide in the reference's association, nothing fused:
 *   start_hit, end_hit   the two endpoint tests (:13-18), inflated by r iff the OBB is not filling
 *   slab_hit             the final predicate 0 <= tMin <= 1 && 0 <= tMax <= 1 (:60) after the
 *                        three axes, each inflated by r, without an earlier rejection
 * and the entry parameter of OBB i is
 *   t_i = 0.0   if start_hit
 *         tMin  else if slab_hit
 *         1.0   else if end_hit   (reachable: an axis with |d| < 1e-6 tests only the start
 *                                  against its faces, :34-41)
 *   else OBB i does not block the edge.
 * t_hit = min_i t_i, and obb is the lowest index i, in the order given to epp_world_create /
 * epp_world_update, that attains it; +inf and -1 when no OBB blocks the edge.  So obb >= 0
 * exactly when epp_check_motions (mode 0) gives flag 0 for that edge and can_pass_gate.  The
 * point s + t_hit (e - s) lies on a closed face of the inflated box and is itself in
 * collision.  A zero t_hit may carry either sign.  Non-finite endpoints go through the same
 * operations (NaN compares false); nothing more is promised for them.
 *
 * epp_motions_first_hit: t_hit[i] (n, device f64) and obb[i] (n, device int32, may be NULL)
 * for each of the n edges s1[i] -> s2[i] (n x 3 f64 each).  Every OBB of the world is visited
 * (no grid or tile filter).  Stream-ordered, no host synchronisation and no allocation; a
 * stale world index is rebuilt first, as by epp_check_motions, so the call can be captured
 * (epp_graph_begin) after epp_world_build_index.  EPP_ERR_INVALID_ARGUMENT (before any device
 * work) for a NULL world, n < 0, can_pass_gate not 0 or 1, or a NULL s1, s2 or t_hit with
 * n > 0; n == 0 launches nothing. */
epp_status epp_motions_first_hit(const epp_world* w, const double* s1, const double* s2, int64_t n,
                                 int32_t can_pass_gate, double* t_hit, int32_t* obb, void* stream);
/* The first hit of every track of a batch in the layout of epp_minsnap_batch, straight from
 * the coefficients, in one launch and without writing a row.  chord[k] (n_tracks, device
 * int64) is epp_traj_sweep_batch's first_invalid[k]: the lowest j whose chord row j -> row
 * j + 1 fails (the same detection code).  t_hit[k] (device f64) and obb[k] (device int32, may
 * be NULL) are what epp_motions_first_hit gives for that chord's two row positions, and
 * time[k] (device f64, may be NULL) = t_j + t_hit * (t_j+1 - t_j) on the time columns
 * epp_sample_batch writes with t0 == NULL: one subtract, one multiply, one add, unfused.  A
 * track without a failing chord, or with fewer than two rows, gives -1, +inf, -1.0, -1.
 * Stream-ordered, no host synchronisation and no allocation; a stale world index is rebuilt
 * first.  EPP_ERR_INVALID_ARGUMENT as epp_traj_sweep_batch, and for a NULL chord or t_hit
 * with n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_traj_first_hit_batch(const epp_world* w, const double* seg_times, const double* coeffs,
                                    const int32_t* wp_offsets, int32_t n_tracks, double dt, int32_t can_pass_gate,
                                    int64_t* chord, double* t_hit, double* time, int32_t* obb, void* stream);

/* ---- gate passage: which gates an edge crosses, and which gates, in order, a fitted track
 * passes and when (device pointers).  No epp_world takes part: gates are given as a frame
 * table, n_gates x 5 f64 on the device, row g = [cx, cy, cz, c, s] with (cx, cy, cz) the gate
 * centre (the gate position plus (0, 0, height[type]), getGateCenterAndNormal,
 * src/OnlineTrajGenerator.cpp:50-70) and c, s = cos(yaw), sin(yaw), computed once on the host;
 * the kernels call no trigonometric function.  half_edge: half the opening's edge (the
 * reference's constant is 0.425).  The edge p1 -> p2 crosses gate g iff
 * (OnlineTrajGenerator::checkGatePassed, src/OnlineTrajGenerator.cpp:228-256), every operation
 * one IEEE fp64 multiply, add, subtract or divide in this association, nothing fused:
 *   t1 = p1 - centre;  g1 = (c*t1.x - s*t1.y,  s*t1.x + c*t1.y,  t1.z)    (same for p2 -> g2)
 *   g1.y < 0  &&  g2.y > 0  &&  |(g1.x + g2.x) / 2| <= half_edge  &&  |(g1.z + g2.z) / 2| <= half_edge
 * From negative to positive gate-frame y only; both inequalities are strict (a point exactly on
 * the gate plane crosses on neither side); NaN compares false.  With a crossing go the plane
 * parameter u = g1.y / (g1.y - g2.y) and the two midpoint offsets the predicate tested.
 *
 * epp_gates_crossed: bit g of mask[i] (n, device uint64) is the predicate of edge s1[i] ->
 * s2[i] (n x 3 f64 each) for gate g; n_gates is 0..64, n_gates == 0 writes zeros.
 * Stream-ordered, no host synchronisation and no allocation, so the call can be captured
 * (epp_graph_begin).  EPP_ERR_INVALID_ARGUMENT (before any device work) for n_gates < 0 or
 * > 64, half_edge negative or not finite, n < 0, or a NULL s1, s2 or mask (or gates with
 * n_gates > 0) with n > 0; n == 0 launches nothing. */
epp_status epp_gates_crossed(const double* gates, int32_t n_gates, double half_edge, const double* s1,
                             const double* s2, int64_t n, uint64_t* mask, void* stream);
/* The ordered gate passage of every track of a batch in the layout of epp_minsnap_batch,
 * straight from the coefficients, in one launch and without writing a row.  Chord j of track k
 * is row j -> row j + 1 of Trajectory::evaluateRange(0, max_time, dt) (positions: columns
 * 0 / 3 / 6 of epp_sample_batch's rows).  With c_-1 = 0, c_g is the smallest j >= c_g-1 whose
 * chord crosses gate g (the same chord may pass consecutive gates; a gate listed twice is
 * found twice on a track that goes round twice); without one, gate g and every later gate are
 * unpassed.  chord[k * n_gates + g] (device int64) = c_g, -1 if unpassed;
 * time[k * n_gates + g] (device f64, may be NULL) = t_j + u * (t_j+1 - t_j) on the time
 * columns epp_sample_batch writes with t0 == NULL (one subtract, one multiply, one add,
 * unfused), -1.0 if unpassed; offset[(k * n_gates + g) * 2 + {0, 1}] (device f64, may be NULL)
 * the two midpoint offsets, NaN if unpassed; n_passed[k] (device int32, required) the number
 * of leading gates passed.  A track with fewer than two rows (one waypoint, the NaN times of a
 * failed fit) passes nothing.  The answers are those of epp_sample_count + epp_sample_batch +
 * epp_gates_crossed(s1 = rows j, s2 = rows j + 1) and the ordered resolution, bit for bit.
 * Stream-ordered, no host synchronisation and no allocation, so the call can be captured.
 * EPP_ERR_INVALID_ARGUMENT (before any device work) as epp_gates_crossed for n_gates and
 * half_edge, for n_tracks < 0, dt <= 0 or not finite, or a NULL seg_times, coeffs, wp_offsets
 * or n_passed (or gates or chord with n_gates > 0) with n_tracks > 0; n_tracks == 0 launches
 * nothing. */
epp_status epp_traj_gate_pass_batch(const double* gates, int32_t n_gates, double half_edge, const double* seg_times,
                                    const double* coeffs, const int32_t* wp_offsets, int32_t n_tracks, double dt,
                                    int64_t* chord, double* time, double* offset, int32_t* n_passed, void* stream);

/* ---- thrust and body rates: what a quadrotor must do to fly a fitted track (device pointers).
 * No epp_world takes part.  The input-feasibility quantities of a differentially flat quadrotor
 * track (Mueller, Hehn, D'Andrea 2015) need the acceleration and the jerk of its rows. */
/* Trajectory::evaluateRange(0, max_time, dt, order) (external/poly_traj/src/trajectory.cpp:
 * 81-141) for every track of a batch in the layout of epp_minsnap_batch: values (total rows x 3
 * f64, [x, y, z]) holds derivative `order` (0..9) of every row; track k is written from row
 * row_offsets[k] on (device int64; a NULL row_offsets: every track from row 0, for one track).
 * The rows are those of epp_sample_count / epp_sample_batch (the same recurrence), and each
 * value is the sampler's own evaluation: the products B[order][j] * c_j rounded once each, then
 * fused Horner steps; so for order 0, 1, 2 the values equal columns 3 d + order of
 * epp_sample_batch's rows bit for bit.  A track without rows (one waypoint, the NaN times of a
 * failed fit) writes nothing.  Stream-ordered, no host synchronisation and no allocation, so
 * the call can be captured (epp_graph_begin).  EPP_ERR_INVALID_ARGUMENT (before any device
 * work) for order outside 0..9, n_tracks < 0, dt <= 0 or not finite, or a NULL seg_times,
 * coeffs, wp_offsets or values with n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_sample_derivative_batch(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                                       int32_t n_tracks, double dt, int32_t order, const int64_t* row_offsets,
                                       double* values, void* stream);
/* Per sample, from its acceleration a and jerk j (acc, jerk: n x 3 f64 each) and the gravity g,
 * every operation one IEEE fp64 multiply, add, subtract, divide or square root in this
 * association, nothing fused:
 *   Fx = ax;  Fy = ay;  Fz = az + g                      (mass-normalised thrust vector)
 *   f2 = (Fx*Fx + Fy*Fy) + Fz*Fz;       thrust   = sqrt(f2)
 *   cx = Fy*jz - Fz*jy;  cy = Fz*jx - Fx*jz;  cz = Fx*jy - Fy*jx
 *   w2 = (cx*cx + cy*cy) + cz*cz;       rate     = sqrt(w2) / f2
 *                                       cos_tilt = Fz / thrust
 * rate = |F x j| / |F|^2 is the angular rate of the thrust direction: the roll / pitch body
 * rate.  No trigonometric function is called: the tilt angle is acos(cos_tilt).  At f2 == 0
 * (free fall) thrust is 0, cos_tilt NaN and rate NaN or +inf, as the operations give;
 * non-finite inputs go through the same operations and nothing more is promised for them.
 * thrust, rate, cos_tilt: n device f64 each; rate and cos_tilt may be NULL.  Stream-ordered, no
 * host synchronisation and no allocation, so the call can be captured (epp_graph_begin).
 * EPP_ERR_INVALID_ARGUMENT (before any device work) for n < 0, a non-finite g, or a NULL acc,
 * jerk or thrust with n > 0; n == 0 launches nothing. */
epp_status epp_thrust_rates(const double* acc, const double* jerk, int64_t n, double g, double* thrust, double* rate,
                            double* cos_tilt, void* stream);
/* The extremes of the three quantities over every track of a batch in the layout of
 * epp_minsnap_batch, straight from the coefficients, in one launch and without writing a row.
 * Over the rows of Trajectory::evaluateRange(0, max_time, dt) of track k, with a and j the
 * order-2 and order-3 values epp_sample_derivative_batch gives:
 *   out[k * 8 + ..] (device f64) = [f_min, t_fmin, f_max, t_fmax, rate_max, t_rate, cos_min, t_cos]
 *   rows[k * 4 + ..] (device int64, may be NULL) = the rows of f_min, f_max, rate_max, cos_min
 * Each extreme is taken over the row values themselves (the rounded thrust, rate, cos_tilt),
 * the earliest row that attains it wins, and a value replaces the running extreme only on
 * strict < or >: a NaN never does, a +inf rate does.  Each t_* is that row's time column as
 * epp_sample_batch writes it with t0 == NULL.  A track without rows (one waypoint, the NaN
 * times of a failed fit) and a quantity that is NaN on every row keep the reductions'
 * identities [+inf, -1, -inf, -1, -inf, -1, +inf, -1] and row -1.  The answers are those of
 * epp_sample_count + epp_sample_batch (the time column), epp_sample_derivative_batch at orders
 * 2 and 3, epp_thrust_rates on those values and the per-track reductions, bit for bit.
 * Stream-ordered, no host synchronisation and no allocation, so the call can be captured.
 * EPP_ERR_INVALID_ARGUMENT (before any device work) as epp_sample_derivative_batch, for a
 * non-finite g, or a NULL out with n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_traj_thrust_rates_batch(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                                       int32_t n_tracks, double dt, double g, double* out, int64_t* rows,
                                       void* stream);

/* ---- time scaling to thrust, body-rate and tilt limits (device pointers).  The reference
 * stretches a track that violates v_max / a_max (Trajectory::scaleSegmentTimesToMeetConstraints,
 * external/poly_traj/src/trajectory.cpp:385-429; epp_traj_scale_to_limits above); these two
 * calls extend that behaviour to the quantities of epp_thrust_rates.  Under x(t / s) the
 * thrust is |a / s^2 + g e_z|, no power of s, so the scale is searched for, not computed.
 * One definition (csrc/thrust_scale.h), every operation one IEEE fp64 operation:
 *   grid points: segment m of time T_m gives tau_i = T_m * (i / 64), i = 0..63, and tau = T_m
 *       (the 65 points epp_traj_peaks looks at); a = p''(tau), j = p'''(tau) of the input track
 *       by Horner over the derivative's coefficients; a point's time is the sum of the earlier
 *       segment times plus tau;
 *   at scale s: s2 = s * s, s3 = s2 * s, a_s = a / s2, j_s = j / s3 (divisions), then the
 *       arithmetic of epp_thrust_rates on (a_s, j_s, g).
 * Like epp_traj_peaks they look at 65 points per segment: a bump narrower than T / 64 can be
 * missed, and the rows every dt of the scaled track are other points than the grid (a caller
 * who needs the rows' answer runs epp_traj_thrust_rates_batch on the result).  Both are
 * stream-ordered, with no host synchronisation and no allocation, so they can be captured. */
/* The four extremes over the grid points of every track at the scale scale_in[k] (device
 * f64; NULL: 1), in epp_traj_thrust_rates_batch's layout:
 *   out[k * 8 + ..] (device f64) = [f_min, t_fmin, f_max, t_fmax, rate_max, t_rate, cos_min, t_cos]
 * The times are in the INPUT track's time (not multiplied by the scale).  A value replaces the
 * running extreme only on strict < or >, ties go to the earliest time, a NaN never wins; a
 * track that is invalid as for epp_traj_peaks (one waypoint, a segment time <= 0, non-finite
 * input) and a quantity that is NaN on every point keep the identities [+inf, -1, -inf, -1,
 * -inf, -1, +inf, -1].  A scale that is not finite and > 0 gives what the operations give.
 * EPP_ERR_INVALID_ARGUMENT (before any device work) for n_tracks < 0, a non-finite g, or a
 * NULL seg_times, coeffs, wp_offsets or out with n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_traj_thrust_grid_batch(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                                      int32_t n_tracks, const double* scale_in, double g, double* out, void* stream);
/* Scales every track of the batch in time, in place, until no grid point violates
 *   thrust < f_min (bit 0) | thrust > f_max (bit 1) | rate > rate_max (bit 2) | cos_tilt < cos_tilt_min (bit 3)
 * (a NaN violates nothing), the whole search and the apply in one launch.  A track feasible at
 * scale 1 comes back bit for bit, scale 1.0, status 0.  Otherwise hi = 2 is doubled while the
 * track is infeasible at hi, up to 1024 (infeasible there: status 1, scale 1.0, the track
 * untouched); then lo = hi / 2 and exactly 12 rounds of mid = 0.5 * (lo + hi), hi = mid when
 * feasible at mid, else lo = mid.  scale[k] = hi is applied as one round of
 * epp_traj_scale_to_limits: T[i] = T[i] * s and every polynomial through
 * scalePolynomialInTime(1 / s).  status[k] (device int32): 0, 1, or -1 for an invalid track
 * (as epp_traj_peaks; untouched, scale 1.0).  violated[k] (device int32, may be NULL): the bits
 * violated at scale 1; 0 for a feasible or invalid track.
 * The limits must satisfy 0 <= f_min < g < f_max, rate_max > 0, cos_tilt_min < 1, g finite and
 * > 0: then every finite track is feasible for a large enough scale (thrust -> g, rate -> 0,
 * cos_tilt -> 1).  f_max = +inf, rate_max = +inf and cos_tilt_min <= -1 switch a limit off,
 * f_min = 0 the lower thrust bound.  Only f_max is monotone in the scale; f_min, the rate and
 * the tilt are not (a track can be feasible at a small scale with its thrust axis pointing
 * down), so the answer is A feasible scale >= 1 with an infeasible one within 2^-12 below it
 * (or exactly 1), not a proven minimum, and a track feasible at 1 is taken as it is.  Scaling
 * alters a non-zero start velocity, as epp_traj_scale_to_limits does.
 * EPP_ERR_INVALID_ARGUMENT (before any device work) for limits outside those conditions, a
 * non-finite g, n_tracks < 0, or a NULL seg_times, coeffs, wp_offsets, scale or status with
 * n_tracks > 0; n_tracks == 0 launches nothing. */
epp_status epp_traj_scale_to_thrust_limits(double* seg_times, double* coeffs, const int32_t* wp_offsets,
                                           int32_t n_tracks, double g, double f_min, double f_max, double rate_max,
                                           double cos_tilt_min, double* scale, int32_t* status, int32_t* violated,
                                           void* stream);

/* ---- segment-time allocation (device pointers) ------------------------------------- */
/* PolynomialOptimization::computeCost (impl/polynomial_optimization_linear_impl.h:123-140) of
 * every track of a batch in the layout of epp_minsnap_batch, from its coefficients:
 *   cost[k] = 0.5 * sum_seg sum_dim c^T Q(T) c,
 *   Q[a][b] = B4[a] B4[b] T^(a+b-7) 2 / (a+b-7) for a, b >= 4, else 0, B4[j] = j! / (j-4)!
 * (computeQuadraticCostJacobian, impl :567-583, derivative 4): the integral of the squared
 * snap over the track.  The order of the arithmetic is csrc/time_alloc.h's.  status (n_tracks,
 * may be NULL): 0 ok; -1 as epp_traj_peaks (no segment, a segment time <= 0 or non-finite
 * input): cost NaN. */
epp_status epp_traj_snap_cost(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                              int32_t n_tracks, double* cost, int32_t* status, void* stream);
/* getCostAndGradientMellinger (impl/polynomial_optimization_nonlinear_impl.h:286-364) of every
 * track at the caller's segment times: cost[k] = J(T), the cost above of the fit at T
 * (epp_minsnap_batch_times), and for every segment n (grad: total segments)
 *   grad[n] = (J(T^(n)) - J(T)) / h,
 *   T^(n)_i = max(t_min, T_i + h) for i = n, max(t_min, T_i - h / (M - 1)) for i != n:
 * a directional difference at constant total time, except that the clamp may change the
 * total; the quotient divides by h all the same, as the reference does (its h and t_min are
 * both 0.1).  A track of one segment has gradient 0.  One workgroup per (track, variant):
 * sum (M + 1) independent solves in one launch.  status (n_tracks, may be NULL): the fit's at
 * T (0, -1, -2, -3: cost and gradient NaN), else -3 when a variant's solve broke down (its
 * gradient entry is NaN).  EPP_ERR_INVALID_ARGUMENT for h <= 0 or t_min <= 0 (or NaN). */
epp_status epp_minsnap_time_gradient(const double* wp, const int32_t* wp_offsets, int32_t n_tracks,
                                     const double* v0, const double* a0, const double* seg_times, double h,
                                     double t_min, double* cost, double* grad, int32_t* status, void* stream);
/* The parameters of epp_minsnap_optimize_times.  h and t_min are the reference's
 * (increment_time and kOptimizationTimeLowerBound, both 0.1); step0, max_halvings, ftol and
 * max_iter are this library's choices: the reference hands the iteration to NLopt. */
typedef struct epp_timeopt_params {
    double h;              /* the gradient's increment, > 0 */
    double t_min;          /* lower bound of every segment time, > 0 */
    double step0;          /* first step: the shortest segment changes by at most this part, in (0, 1] */
    int32_t max_halvings;  /* halvings of a rejected step, >= 0 */
    double ftol;           /* stop when a step lowers the cost by <= ftol * cost, >= 0 */
    int32_t max_iter;      /* accepted steps at most, >= 0 */
} epp_timeopt_params;
#define EPP_TIMEOPT_DEFAULTS {0.1, 0.1, 0.5, 8, 1e-4, 20}
/* Redistributes every track's duration over its segments to lower the snap cost, the total
 * kept: the outer loop of Mellinger's time allocation, the whole loop of a track in one
 * launch (one workgroup per track, its solves one after another; the batch is the
 * parallelism).  seg_times: in the start, out the result; coeffs (out): the fit at the result,
 * bit for bit epp_minsnap_batch_times there.  Per iteration, with J and g as
 * epp_minsnap_time_gradient(h, t_min) gives them at T:
 *   d_i = g_i - (sum_{n != i} g_n) / (M - 1)        (sums to 0: the total is kept)
 *   stop, status 0, when max_i |d_i| == 0; stop, status 1, when some d_i is not finite
 *   alpha = step0 * min_i T_i / max_i |d_i|
 *   try T' = T - alpha d, at most 1 + max_halvings times, alpha halved after each failure,
 *   until every T'_i >= t_min and J(T') < J(T); none accepted: stop, status 1
 *   T = T'; stop, status 0, when J(T) - J(T') <= ftol * J(T)
 * and status 2 after max_iter accepted steps.  Then T is multiplied by (starting sum) / (sum
 * of T), both sums in order, and fitted once more: that solve's coefficients and cost are the
 * outputs.  cost0 / cost1 (n_tracks): the cost at the start and of the result; iters: the
 * accepted steps.  A track of one segment, max_iter == 0 and a track whose first fit fails
 * or is not finite return the plain fit at the given times: cost1 == cost0, iters 0, status
 * the fit's (0, -1, -2, -3).  EPP_ERR_INVALID_ARGUMENT for h <= 0, t_min <= 0, step0 outside
 * (0, 1], ftol < 0 (or NaN), max_halvings < 0 or max_iter < 0. */
epp_status epp_minsnap_optimize_times(const double* wp, const int32_t* wp_offsets, int32_t n_tracks,
                                      const double* v0, const double* a0, double* seg_times, double* coeffs,
                                      epp_timeopt_params params, double* cost0, double* cost1, int32_t* iters,
                                      int32_t* status, void* stream);

/* ---- batch planner building blocks (device pointers) ------------------------------- */
/* Replace OMPL's sampler / nearest-neighbour structure behind PathPlanner::planPath
 * (src/PathPlanner.cpp:80-158).  Counter-based uniform states in [lo, hi]:
 * u = (splitmix64(seed ^ (3 (start + i) + d)) >> 11) * 2^-53, x_d = lo_d + (hi_d - lo_d) u. */
epp_status epp_sample_uniform(uint64_t seed, const double lo[3], const double hi[3], int64_t n,
                              int64_t start, double* xyz, void* stream);
/* k nearest neighbours (k in {4, 8, 16, 32}) of every node within max_dist (<= 0: no
 * limit), sorted by distance, ties to the lower index; missing entries are -1.  The radius is
 * exclusive on every path: node j is in range of node i iff the squared distance
 * (dx^2 + dy^2) + dz^2, in double, is < max_dist^2; a neighbour at exactly max_dist is not. */
epp_status epp_knn(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* stream);
/* The two strategies behind epp_knn (same answers): all-pairs with LDS tiles, and a
 * uniform grid walked in shells. */
epp_status epp_knn_bruteforce(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr,
                              void* stream);
epp_status epp_knn_grid(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* stream);
/* Caller-workspace variants (no allocation, no cross-stream ordering inside): `ws` is a
 * 256-byte aligned device buffer of at least epp_knn_workspace_size(n) bytes that no
 * other stream touches until this call's kernels completed.  Its prior contents do not
 * matter (the call clears what it reads before writing it).  epp_knn / epp_knn_grid
 * use a cached per-device workspace whose reuse is ordered by a completion event. */
uint64_t epp_knn_workspace_size(int32_t n);
epp_status epp_knn_ws(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* ws,
                      uint64_t ws_bytes, void* stream);
epp_status epp_knn_grid_ws(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* ws,
                           uint64_t ws_bytes, void* stream);
/* The same with the grid laid over the caller's box [lo, hi] (host arrays) instead of the
 * nodes' bounding box, which saves its device reduction (two kernels fewer): every node
 * must lie inside the closed box (the planner's samples lie in the world bounds; start and
 * goal widen them).  Same answers.  Precondition, not checked: a node outside the box is
 * clamped into a boundary cell, which breaks the search's distance bounds, and the table is
 * then unspecified (not necessarily exact). */
epp_status epp_knn_ws_box(const double* nodes, int32_t n, int32_t k, double max_dist, const double lo[3],
                          const double hi[3], int32_t* nbr, void* ws, uint64_t ws_bytes, void* stream);
epp_status epp_knn_grid_ws_box(const double* nodes, int32_t n, int32_t k, double max_dist, const double lo[3],
                               const double hi[3], int32_t* nbr, void* ws, uint64_t ws_bytes, void* stream);
/* Edge endpoints for every (node i, neighbour c): s1 = nodes[i], s2 = nodes[nbr[i k + c]]
 * (s2 = s1 for a missing neighbour).  s1, s2: n k x 3. */
epp_status epp_knn_edges(const double* nodes, const int32_t* nbr, int32_t n, int32_t k, double* s1,
                         double* s2, void* stream);
/* The motion checks of a k-NN table without materialising its edges: valid[e] for edge e
 * from node e / k to node nbr[e] (a missing neighbour, -1: the degenerate edge to itself),
 * as epp_check_motions on epp_knn_edges' output would give.  EPP_ERR_UNSUPPORTED when the
 * batch or world is not for the tile-filtered kernel (small batches, worlds without tile
 * tables): then use epp_knn_edges + epp_check_motions. */
epp_status epp_check_knn_motions(const epp_world* w, const double* nodes, const int32_t* nbr, int32_t n, int32_t k,
                                 int32_t can_pass_gate, int32_t mode, uint8_t* valid, void* stream);
/* Ordered stream compaction of the valid states (planner node list): out = xyz[i] for
 * valid[i] != 0, in index order; *n_out (device int64) = their count.  out holds n x 3. */
epp_status epp_compact_states(const double* xyz, const uint8_t* valid, int64_t n, double* out, int64_t* n_out,
                              void* stream);
/* Caller-workspace variant (ws: >= epp_compact_workspace_size(n) device bytes that no
 * other stream uses until this call's kernels completed; any prior contents: the call
 * zeroes its look-back status words first); epp_compact_states uses a
 * cached per-device workspace ordered by an event (serialising concurrent streams). */
uint64_t epp_compact_workspace_size(int64_t n);
epp_status epp_compact_states_ws(const double* xyz, const uint8_t* valid, int64_t n, double* out, int64_t* n_out,
                                 void* ws, uint64_t ws_bytes, void* stream);
/* nbr[e] = -1 where valid[e] == 0 (edges that failed the motion check), in place. */
epp_status epp_mask_edges(int32_t* nbr, const uint8_t* valid, int64_t m, void* stream);
/* The same, and count[0..1] (device memory, set by the call) = the entries of nbr that are
 * >= 0 afterwards and those equal to `target` (the planner's valid-edge statistic and the
 * goal's incoming edges, without a host pass over nbr). */
epp_status epp_mask_edges_count(int32_t* nbr, const uint8_t* valid, int64_t m, int32_t target, int64_t* count,
                                void* stream);

/* ---- multi-GPU: the multi-track plan's exchange step (RCCL over xGMI) --------------- */
/* BASELINE config 4 / SURVEY §8e: every rank (one GPU) plans its own track; the final
 * waypoint sets are then all-gathered.  No reference counterpart (the reference is
 * single-threaded CPU code).  RCCL is loaded at first use (librccl.so.1); without it these
 * return EPP_ERR_UNSUPPORTED.
 * One process per GPU: rank 0 calls epp_comm_unique_id and shares the 128 bytes out of
 * band (bench.py: a file rendezvous, eppamd/dist.py; or MPI, torch.distributed); every
 * rank calls epp_comm_init on its device.
 * One process, several GPUs: epp_comm_init_all (one communicator per device; use each
 * from its own host thread). */
typedef struct epp_comm epp_comm;
/* EPP_OK if RCCL can be loaded in this process (no communicator is created). */
epp_status epp_comm_available(void);
epp_status epp_comm_unique_id(uint8_t id[128]);
epp_status epp_comm_init(const uint8_t id[128], int32_t n_ranks, int32_t rank, epp_comm** out);
epp_status epp_comm_init_all(int32_t n_devices, const int32_t* devices, epp_comm** out /* n_devices */);
epp_status epp_comm_destroy(epp_comm* comm);
epp_status epp_comm_rank(const epp_comm* comm, int32_t* rank, int32_t* n_ranks);
/* Failure safety of every collective below: the call never blocks inside RCCL.  While its
 * collective runs it polls RCCL's asynchronous error state (a peer process died, a broken
 * connection), an abort requested with epp_comm_abort, and a deadline (default 120 s,
 * epp_comm_set_timeout).  On any of them it aborts the communicator (ncclCommAbort) and
 * returns EPP_ERR_PEER (error, abort) or EPP_ERR_TIMEOUT; every later call on that
 * communicator returns EPP_ERR_PEER at once (destroy it and create a new one).
 * epp_comm_abort may be called from any thread (e.g. by the owner of another rank's
 * communicator in the same process when that rank failed locally). */
epp_status epp_comm_set_timeout(epp_comm* comm, double seconds);
epp_status epp_comm_abort(epp_comm* comm);
/* All-gather of every rank's waypoint set (wp: n x 3 HOST doubles): counts[r] = rank r's
 * count (n_ranks entries), out + r * cap * 3 = its points (HOST, n_ranks x cap x 3).  Every
 * rank must call it, also a rank that has no set because its own work failed: it passes
 * n = -1 (wp may be NULL).  Every rank then returns EPP_ERR_PEER with counts filled (-1
 * marks the failed ranks) and the sets are not exchanged, so one rank's failure ends the
 * exchange on all ranks instead of leaving them in the collective.  EPP_ERR_CAPACITY
 * (counts filled, on every rank) if a rank has more than cap. */
epp_status epp_comm_allgather_waypoints(epp_comm* comm, const double* wp, int32_t n, int32_t cap, double* out,
                                        int32_t* counts);
/* x[0..n) (HOST doubles, in place) reduced over the ranks: op EPP_REDUCE_SUM / MAX / MIN.
 * The max-over-ranks timing and the collective error flags of a multi-rank caller. */
#define EPP_REDUCE_SUM 0
#define EPP_REDUCE_MAX 1
#define EPP_REDUCE_MIN 2
epp_status epp_comm_allreduce_f64(epp_comm* comm, double* x, int32_t n, int32_t op);
/* Returns once every rank has called it (an all-reduce of one double). */
epp_status epp_comm_barrier(epp_comm* comm);

/* ---- host-buffer convenience (synchronous; used by the C++ API shims) ------------- */
/* generateTrajectory for one track with host buffers (poly_traj::generateTrajectory,
 * external/poly_traj/src/trajectory_generator.cpp:12-100): one fused launch (min-snap
 * solve + evaluateRange sampling) reading and writing pinned host memory.  Returns the row
 * count in *n_rows; rows is allocated with malloc and must be released with
 * epp_host_free.  EPP_ERR_INVALID_ARGUMENT "At least two waypoints are required";
 * EPP_ERR_RUNTIME "Segment times need to be greater than zero" (the reference's glog
 * CHECK). */
epp_status epp_generate_trajectory_host(const double* wp, int32_t n_wp, double v_max, double a_max,
                                        double dt, double t0, const double v0[3], const double a0[3],
                                        double** rows, int64_t* n_rows);
/* The same with the caller's segment times (n_wp - 1 of them) instead of Nfabian's. */
epp_status epp_generate_trajectory_times_host(const double* wp, int32_t n_wp, const double* seg_times, double dt,
                                              double t0, const double v0[3], const double a0[3], double** rows,
                                              int64_t* n_rows);
/* The same under the caller's constraints (epp_minsnap_batch_constrained above: fixed_mask
 * n_wp bytes, fixed_val n_wp x 12, HOST arrays here): the constrained fit at seg_times
 * (n_wp - 1 of them, NULL: Nfabian times under v_max / a_max), then evaluateRange sampling.
 * Two launches over pinned host buffers; the rows are those of epp_sample_batch on
 * epp_minsnap_batch_constrained's output.  Errors as epp_generate_trajectory_host; also
 * EPP_ERR_INVALID_ARGUMENT for a mask bit above bit 3 or a non-finite value in a used slot. */
epp_status epp_generate_trajectory_constrained_host(const double* wp, int32_t n_wp, double v_max, double a_max,
                                                    const double* seg_times, double dt, double t0,
                                                    const uint8_t* fixed_mask, const double* fixed_val,
                                                    double** rows, int64_t* n_rows);
/* epp_generate_trajectory_host with v_max and a_max enforced on the fitted trajectory:
 * fit, then Trajectory::scaleSegmentTimesToMeetConstraints (external/poly_traj/src/
 * trajectory.cpp:385-429; epp_traj_scale_to_limits above), then evaluateRange sampling of
 * the scaled trajectory (the row count follows the scaled times).  Three launches over
 * pinned host buffers; the fit is the batch kernel's (epp_minsnap_batch), so the rows are
 * those of epp_sample_batch on epp_traj_scale_to_limits' output.  *scale_out (may be
 * NULL): the factor applied to the segment times (1.0: the fit was within the limits).
 * Errors as epp_generate_trajectory_host; also EPP_ERR_INVALID_ARGUMENT for v_max <= 0 or
 * a_max <= 0, EPP_ERR_RUNTIME when the limits are not met after 20 rounds. */
epp_status epp_generate_trajectory_limited_host(const double* wp, int32_t n_wp, double v_max, double a_max,
                                                double dt, double t0, const double v0[3], const double a0[3],
                                                double** rows, int64_t* n_rows, double* scale_out);
/* epp_generate_trajectory_host made flyable: the fit, then epp_traj_scale_to_limits when
 * enforce_va != 0, then epp_traj_scale_to_thrust_limits under (g, f_min, f_max, rate_max,
 * cos_tilt_min), then the sampling of the scaled trajectory.  Scaling up keeps |v| and |a|
 * within their limits, so that order is safe.  Launches over pinned host buffers as
 * epp_generate_trajectory_limited_host; the rows are those of epp_sample_batch on the two
 * calls' output.  *scale_va, *scale_thrust (may be NULL): the two factors applied (1.0: none).
 * Errors as epp_generate_trajectory_limited_host (v_max, a_max > 0 are asked for only when
 * enforce_va); also EPP_ERR_INVALID_ARGUMENT for limits epp_traj_scale_to_thrust_limits
 * rejects, EPP_ERR_RUNTIME when the track is still infeasible at scale 1024. */
epp_status epp_generate_trajectory_flyable_host(const double* wp, int32_t n_wp, double v_max, double a_max,
                                                double dt, double t0, const double v0[3], const double a0[3],
                                                int32_t enforce_va, double g, double f_min, double f_max,
                                                double rate_max, double cos_tilt_min, double** rows,
                                                int64_t* n_rows, double* scale_va, double* scale_thrust);
/* epp_generate_trajectory_host with the segment times optimised before anything else: the
 * Nfabian fit, epp_minsnap_optimize_times under `params`, then -- uniform scaling keeps the
 * optimised ratios -- epp_traj_scale_to_limits when enforce_va != 0 and
 * epp_traj_scale_to_thrust_limits when thrust_limits ([g, f_min, f_max, rate_max,
 * cos_tilt_min], may be NULL) is given, then the sampling; one stream, launches over pinned
 * host buffers as epp_generate_trajectory_limited_host.  *cost0, *cost1, *iters (may be NULL):
 * the descent's.  Errors as epp_generate_trajectory_flyable_host and
 * epp_minsnap_optimize_times. */
epp_status epp_generate_trajectory_timeopt_host(const double* wp, int32_t n_wp, double v_max, double a_max,
                                                double dt, double t0, const double v0[3], const double a0[3],
                                                epp_timeopt_params params, int32_t enforce_va,
                                                const double* thrust_limits, double** rows, int64_t* n_rows,
                                                double* cost0, double* cost1, int32_t* iters);
/* The C5 online step's two GPU calls in ONE launch (an addition of this build; the
 * reference makes them one after the other: PathPlanner::checkTrajectoryValidity,
 * src/PathPlanner.cpp:267-280, then poly_traj::generateTrajectory, src/
 * OnlineTrajGenerator.cpp:374-379): check_valid[i] = World::checkPointValidity(check_xyz[i],
 * min_distance) (src/World.cpp:106-128) for the n_check points (HOST array, e.g. the
 * lookahead rows' positions) against `world`, and the trajectory of epp_generate_trajectory_host.
 * The check runs on extra workgroups of the refit's kernel: one pinned upload, one
 * completion poll.  Same answers as the two calls.  The check must be small (n_check <=
 * 4096, <= 256 OBBs), else EPP_ERR_UNSUPPORTED (make the two calls). */
epp_status epp_check_and_generate_trajectory_host(const epp_world* world, const double* check_xyz, int64_t n_check,
                                                  double min_distance, uint8_t* check_valid, const double* wp,
                                                  int32_t n_wp, double v_max, double a_max, double dt, double t0,
                                                  const double v0[3], const double a0[3], double** rows_out,
                                                  int64_t* n_rows);
/* The "optimal" trajectory type (OptimalTimeParametrizer::calculateTrajectory,
 * external/time_parametrization/src/OptimalTimeParametrizer.cpp:11-108; host code: one
 * sequential phase-plane integration).  wp: n_wp x 3, pre: n_pre x 3 lead-in points
 * (may be NULL when n_pre = 0).  rows: *n_rows x 11 [x vx ax y vy ay z vz az yaw t+t0],
 * malloc'd, release with epp_host_free.  EPP_ERR_RUNTIME "Trajectory is not valid" when
 * the integration fails. */
epp_status epp_optimal_trajectory_host(const double* wp, int32_t n_wp, const double* pre, int32_t n_pre,
                                       double v_max, double a_max, double dt, double t0, double max_deviation,
                                       double** rows, int64_t* n_rows);
/* The "spline" trajectory type (TrajInterpolation::interpolateTraj,
 * src/TrajInterpolation.cpp:44-68): cubic B-spline through wp (n_wp >= 4) at chord-length
 * parameters, int((max_t - t0) / dt) + 1 rows [x 0 0 y 0 0 z 0 0 t], t = i dt + t0;
 * malloc'd, release with epp_host_free. */
epp_status epp_spline_trajectory_host(const double* wp, int32_t n_wp, double max_t, double t0, double dt,
                                      double** rows, int64_t* n_rows);
void epp_host_free(void* p);

#ifdef __cplusplus
}
#endif

#endif /* EPP_H_ */
