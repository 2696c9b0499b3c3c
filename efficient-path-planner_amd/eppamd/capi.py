"""ctypes binding of the C ABI in include/epp.h (libepp.so, built in-tree).

This is the product path: every call goes to the HIP kernels in libepp.so.  There is
no CPU fallback — if the library or a GPU is missing the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# EPP_LIB: another build of the same ABI (diagnostics A/B builds under scripts/dbg/)
LIB_PATH = os.environ.get("EPP_LIB") or os.path.join(os.path.dirname(_HERE), "libepp.so")

OBB_DTYPE = np.dtype([("center", "<f8", 3), ("half", "<f8", 3), ("rot", "<f8", 9),
                      ("filling", "<i4"), ("is_gate", "<i4")])

EPP_OK = 0
EPP_ERR_INVALID_ARGUMENT = -1
EPP_ERR_RUNTIME = -2
EPP_ERR_HIP = -3
EPP_ERR_UNSUPPORTED = -4
EPP_ERR_CAPACITY = -5
EPP_ERR_PEER = -6
EPP_ERR_TIMEOUT = -7
EPP_REDUCE_SUM, EPP_REDUCE_MAX, EPP_REDUCE_MIN = 0, 1, 2

_lib = None


class EppError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"epp error {code}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run __graft_entry__.build()")
        l = C.CDLL(LIB_PATH)
        vp, i32, i64, u64, dp = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
        sig = {
            "epp_last_error": (C.c_char_p, []),
            "epp_version": (C.c_char_p, []),
            "epp_device_count": (i32, [C.POINTER(C.c_int)]),
            "epp_set_device": (i32, [C.c_int]),
            "epp_device_cu_count": (i32, [C.POINTER(C.c_int)]),
            "epp_malloc": (i32, [C.POINTER(vp), u64]),
            "epp_free": (i32, [vp]),
            "epp_memcpy_h2d": (i32, [vp, vp, u64, vp]),
            "epp_memcpy_d2h": (i32, [vp, vp, u64, vp]),
            "epp_memcpy_h2d_async": (i32, [vp, vp, u64, vp]),
            "epp_memcpy_d2h_async": (i32, [vp, vp, u64, vp]),
            "epp_memset": (i32, [vp, C.c_int, u64, vp]),
            "epp_stream_create": (i32, [C.POINTER(vp)]),
            "epp_stream_destroy": (i32, [vp]),
            "epp_stream_sync": (i32, [vp]),
            "epp_device_sync": (i32, []),
            "epp_event_create": (i32, [C.POINTER(vp)]),
            "epp_event_destroy": (i32, [vp]),
            "epp_event_record": (i32, [vp, vp]),
            "epp_event_elapsed_ms": (i32, [vp, vp, C.POINTER(C.c_float)]),
            "epp_graph_begin": (i32, [vp]),
            "epp_graph_end": (i32, [vp, C.POINTER(vp)]),
            "epp_graph_launch": (i32, [vp, vp]),
            "epp_graph_destroy": (i32, [vp]),
            "epp_build_obbs": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, C.POINTER(i32)]),
            "epp_world_create": (i32, [vp, i32, dp, dp, C.POINTER(vp)]),
            "epp_world_update": (i32, [vp, vp, i32]),
            "epp_world_destroy": (i32, [vp]),
            "epp_world_num_obbs": (i32, [vp, C.POINTER(i32)]),
            "epp_world_get_aabbs": (i32, [vp, vp]),
            "epp_world_generation": (i32, [vp, C.POINTER(C.c_uint64)]),
            "epp_world_build_index": (i32, [vp]),
            "epp_comm_unique_id": (i32, [vp]),
            "epp_comm_init": (i32, [vp, i32, i32, C.POINTER(vp)]),
            "epp_comm_init_all": (i32, [i32, vp, vp]),
            "epp_comm_destroy": (i32, [vp]),
            "epp_comm_rank": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
            "epp_comm_allgather_waypoints": (i32, [vp, vp, i32, i32, vp, vp]),
            "epp_comm_allreduce_f64": (i32, [vp, vp, i32, i32]),
            "epp_comm_barrier": (i32, [vp]),
            "epp_comm_set_timeout": (i32, [vp, dp]),
            "epp_comm_abort": (i32, [vp]),
            "epp_comm_available": (i32, []),
            "epp_check_states": (i32, [vp, vp, i64, i32, vp, vp, vp, vp]),
            "epp_check_states_mindist": (i32, [vp, vp, i64, dp, vp, vp]),
            "epp_check_motions": (i32, [vp, vp, vp, i64, i32, i32, vp, vp]),
            "epp_minsnap_batch": (i32, [vp, vp, i32, dp, dp, vp, vp, vp, vp, vp, vp]),
            "epp_minsnap_batch_times": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, vp]),
            "epp_minsnap_batch_constrained": (i32, [vp, vp, i32, dp, dp, vp, vp, vp, vp, vp, vp, vp]),
            "epp_generate_trajectory_constrained_host": (i32, [vp, i32, dp, dp, vp, dp, dp, vp, vp,
                                                               C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64)]),
            "epp_sample_count": (i32, [vp, vp, i32, dp, vp, vp]),
            "epp_sample_batch": (i32, [vp, vp, vp, i32, dp, vp, vp, vp, vp]),
            "epp_traj_peaks": (i32, [vp, vp, vp, i32, vp, vp, vp]),
            "epp_traj_scale_to_limits": (i32, [vp, vp, vp, i32, dp, dp, vp, vp, vp]),
            "epp_traj_check_batch": (i32, [vp, vp, vp, vp, i32, dp, dp, vp, vp, vp]),
            "epp_traj_sweep_batch": (i32, [vp, vp, vp, vp, i32, dp, i32, vp, vp, vp]),
            "epp_states_clearance": (i32, [vp, vp, i64, vp, vp, vp]),
            "epp_traj_clearance_batch": (i32, [vp, vp, vp, vp, i32, dp, vp, vp, vp, vp, vp]),
            "epp_motions_clearance": (i32, [vp, vp, vp, i64, vp, vp, vp, vp]),
            "epp_traj_chord_clearance_batch": (i32, [vp, vp, vp, vp, i32, dp, vp, vp, vp, vp, vp, vp]),
            "epp_motions_first_hit": (i32, [vp, vp, vp, i64, i32, vp, vp, vp]),
            "epp_traj_first_hit_batch": (i32, [vp, vp, vp, vp, i32, dp, i32, vp, vp, vp, vp, vp]),
            "epp_gates_crossed": (i32, [vp, i32, dp, vp, vp, i64, vp, vp]),
            "epp_traj_gate_pass_batch": (i32, [vp, i32, dp, vp, vp, vp, i32, dp, vp, vp, vp, vp, vp]),
            "epp_sample_derivative_batch": (i32, [vp, vp, vp, i32, dp, i32, vp, vp, vp]),
            "epp_thrust_rates": (i32, [vp, vp, i64, dp, vp, vp, vp, vp]),
            "epp_traj_thrust_rates_batch": (i32, [vp, vp, vp, i32, dp, dp, vp, vp, vp]),
            "epp_traj_thrust_grid_batch": (i32, [vp, vp, vp, i32, vp, dp, vp, vp]),
            "epp_traj_scale_to_thrust_limits": (i32, [vp, vp, vp, i32, dp, dp, dp, dp, dp, vp, vp, vp, vp]),
            "epp_traj_snap_cost": (i32, [vp, vp, vp, i32, vp, vp, vp]),
            "epp_minsnap_time_gradient": (i32, [vp, vp, i32, vp, vp, vp, dp, dp, vp, vp, vp, vp]),
            "epp_minsnap_optimize_times": (i32, [vp, vp, i32, vp, vp, vp, vp, TimeoptParams, vp, vp, vp, vp, vp]),
            "epp_generate_trajectory_timeopt_host": (i32, [vp, i32, dp, dp, dp, dp, vp, vp, TimeoptParams, i32, vp,
                                                           C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64),
                                                           C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                           C.POINTER(i32)]),
            "epp_generate_trajectory_flyable_host": (i32, [vp, i32, dp, dp, dp, dp, vp, vp, i32, dp, dp, dp, dp, dp,
                                                           C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64),
                                                           C.POINTER(C.c_double), C.POINTER(C.c_double)]),
            "epp_generate_trajectory_limited_host": (i32, [vp, i32, dp, dp, dp, dp, vp, vp,
                                                           C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64),
                                                           C.POINTER(C.c_double)]),
            "epp_check_and_generate_trajectory_host": (i32, [vp, vp, i64, dp, vp, vp, i32, dp, dp, dp, dp, vp, vp,
                                                               C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64)]),
            "epp_generate_trajectory_host": (i32, [vp, i32, dp, dp, dp, dp, vp, vp,
                                                   C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64)]),
            "epp_generate_trajectory_times_host": (i32, [vp, i32, vp, dp, dp, vp, vp,
                                                         C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64)]),
            "epp_optimal_trajectory_host": (i32, [vp, i32, vp, i32, dp, dp, dp, dp, dp,
                                                  C.POINTER(C.POINTER(C.c_double)), C.POINTER(i64)]),
            "epp_spline_trajectory_host": (i32, [vp, i32, dp, dp, dp, C.POINTER(C.POINTER(C.c_double)),
                                                 C.POINTER(i64)]),
            "epp_host_free": (None, [vp]),
            "epp_sample_uniform": (i32, [C.c_uint64, vp, vp, i64, i64, vp, vp]),
            "epp_knn": (i32, [vp, i32, i32, dp, vp, vp]),
            "epp_knn_bruteforce": (i32, [vp, i32, i32, dp, vp, vp]),
            "epp_knn_grid": (i32, [vp, i32, i32, dp, vp, vp]),
            "epp_knn_workspace_size": (C.c_uint64, [i32]),
            "epp_knn_ws": (i32, [vp, i32, i32, dp, vp, vp, C.c_uint64, vp]),
            "epp_knn_grid_ws": (i32, [vp, i32, i32, dp, vp, vp, C.c_uint64, vp]),
            "epp_knn_ws_box": (i32, [vp, i32, i32, dp, vp, vp, vp, vp, C.c_uint64, vp]),
            "epp_knn_grid_ws_box": (i32, [vp, i32, i32, dp, vp, vp, vp, vp, C.c_uint64, vp]),
            "epp_knn_edges": (i32, [vp, vp, i32, i32, vp, vp, vp]),
            "epp_compact_states": (i32, [vp, vp, i64, vp, vp, vp]),
            "epp_compact_workspace_size": (C.c_uint64, [i64]),
            "epp_compact_states_ws": (i32, [vp, vp, i64, vp, vp, vp, C.c_uint64, vp]),
            "epp_mask_edges": (i32, [vp, vp, i64, vp]),
            "epp_mask_edges_count": (i32, [vp, vp, i64, i32, vp, vp]),
            "epp_check_knn_motions": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
            # debug entries (csrc/host_dbg_planner.cpp; not in include/epp.h)
            "epp_dbg_plan_batch": (i32, [vp, i32, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32,
                                         vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, vp, vp]),
            "epp_dbg_reverse_csr": (i32, [vp, i32, i32, vp, vp, vp]),
            "epp_dbg_knn_motions_masked": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, vp]),
            "epp_dbg_knn_motions_rows_supported": (i32, [vp]),
            "epp_dbg_knn_motions_rows": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, i32,
                                               i32, vp]),
        }
        for name, (res, args) in sig.items():
            if os.environ.get("EPP_LIB") and not hasattr(l, name):
                continue  # (an A/B build from before the symbol existed)
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


# every symbol include/epp.h declares (the CPU test checks the library exports them)
EXPORTED = [
    "epp_last_error", "epp_version", "epp_device_count", "epp_set_device", "epp_malloc", "epp_free",
    "epp_memcpy_h2d", "epp_memcpy_d2h", "epp_memcpy_h2d_async", "epp_memcpy_d2h_async", "epp_memset", "epp_stream_create", "epp_stream_destroy",
    "epp_stream_sync", "epp_device_sync", "epp_event_create", "epp_event_destroy", "epp_event_record",
    "epp_event_elapsed_ms", "epp_build_obbs", "epp_world_create", "epp_world_update",
    "epp_world_destroy", "epp_world_num_obbs", "epp_world_get_aabbs", "epp_check_states",
    "epp_check_states_mindist", "epp_check_motions", "epp_minsnap_batch", "epp_sample_count",
    "epp_sample_batch", "epp_generate_trajectory_host", "epp_host_free", "epp_sample_uniform", "epp_knn",
    "epp_knn_bruteforce", "epp_knn_grid", "epp_knn_workspace_size", "epp_knn_ws", "epp_knn_grid_ws",
    "epp_knn_edges", "epp_compact_states", "epp_mask_edges", "epp_mask_edges_count", "epp_check_knn_motions", "epp_optimal_trajectory_host",
    "epp_spline_trajectory_host", "epp_compact_workspace_size", "epp_compact_states_ws",
    "epp_graph_begin", "epp_graph_end", "epp_graph_launch", "epp_graph_destroy", "epp_minsnap_batch_times",
    "epp_generate_trajectory_times_host", "epp_world_generation", "epp_world_build_index", "epp_comm_unique_id", "epp_comm_init",
    "epp_comm_init_all", "epp_comm_destroy", "epp_comm_rank", "epp_comm_allgather_waypoints",
    "epp_comm_allreduce_f64", "epp_comm_barrier", "epp_comm_available", "epp_knn_ws_box", "epp_knn_grid_ws_box",
    "epp_comm_set_timeout", "epp_comm_abort", "epp_check_and_generate_trajectory_host",
    "epp_traj_peaks", "epp_traj_scale_to_limits", "epp_generate_trajectory_limited_host",
    "epp_traj_check_batch", "epp_traj_sweep_batch", "epp_states_clearance", "epp_traj_clearance_batch",
    "epp_motions_first_hit", "epp_traj_first_hit_batch", "epp_gates_crossed", "epp_traj_gate_pass_batch",
    "epp_sample_derivative_batch", "epp_thrust_rates", "epp_traj_thrust_rates_batch", "epp_device_cu_count",
    "epp_traj_thrust_grid_batch", "epp_traj_scale_to_thrust_limits", "epp_generate_trajectory_flyable_host",
    "epp_traj_snap_cost", "epp_minsnap_time_gradient", "epp_minsnap_optimize_times",
    "epp_generate_trajectory_timeopt_host", "epp_minsnap_batch_constrained",
    "epp_generate_trajectory_constrained_host", "epp_motions_clearance", "epp_traj_chord_clearance_batch",
]


class TimeoptParams(C.Structure):
    """epp_timeopt_params (include/epp.h); the defaults are EPP_TIMEOPT_DEFAULTS."""
    _fields_ = [("h", C.c_double), ("t_min", C.c_double), ("step0", C.c_double), ("max_halvings", C.c_int32),
                ("ftol", C.c_double), ("max_iter", C.c_int32)]

    def __init__(self, h=0.1, t_min=0.1, step0=0.5, max_halvings=8, ftol=1e-4, max_iter=20):
        super().__init__(float(h), float(t_min), float(step0), int(max_halvings), float(ftol), int(max_iter))


def check(rc: int) -> None:
    if rc != EPP_OK:
        raise EppError(rc, lib().epp_last_error().decode())


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


class DeviceBuffer:
    """A raw HBM allocation (epp_malloc)."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().epp_malloc(C.byref(p), max(int(nbytes), 16)))
        self.ptr = p.value
        self.nbytes = int(nbytes)

    @classmethod
    def from_array(cls, a: np.ndarray, stream=None) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        b.upload(a, stream)
        return b

    def upload(self, a: np.ndarray, stream=None) -> None:
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        check(lib().epp_memcpy_h2d(self.ptr, _ptr(a), a.nbytes, stream))

    def download(self, dtype, count: int, stream=None) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib().epp_memcpy_d2h(_ptr(out), self.ptr, out.nbytes, stream))
        return out

    def zero(self, stream=None) -> None:
        check(lib().epp_memset(self.ptr, 0, self.nbytes, stream))

    def free(self) -> None:
        if self.ptr:
            lib().epp_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_count() -> int:
    n = C.c_int(0)
    check(lib().epp_device_count(C.byref(n)))
    return n.value


def cu_count() -> int:
    """The compute units of the current device (epp_device_cu_count)."""
    n = C.c_int(0)
    check(lib().epp_device_cu_count(C.byref(n)))
    return n.value


def sync() -> None:
    check(lib().epp_device_sync())


def build_obbs(geom, gates: np.ndarray, obstacles: np.ndarray) -> np.ndarray:
    """World::addGate / addObstacle (src/World.cpp:13-55) on the host."""
    gates = np.ascontiguousarray(np.asarray(gates, np.float64).reshape(-1, 7))
    obstacles = np.ascontiguousarray(np.asarray(obstacles, np.float64).reshape(-1, 6))
    cap = len(gates) * max(1, len(geom.gate_desc)) + len(obstacles) * max(1, len(geom.obst_desc))
    out = np.zeros(max(cap, 1), OBB_DTYPE)
    n = C.c_int32(0)
    check(lib().epp_build_obbs(_ptr(geom.gate_desc), _ptr(geom.gate_desc_off), len(geom.gate_desc_off) - 1,
                               _ptr(geom.obst_desc), len(geom.obst_desc), _ptr(gates), len(gates),
                               _ptr(obstacles), len(obstacles), _ptr(out), len(out), C.byref(n)))
    return out[: n.value].copy()


class World:
    """Device-resident OBB table + cull grid (epp_world)."""

    def __init__(self, obbs: np.ndarray, r_gate: float, r_obst: float):
        obbs = np.ascontiguousarray(obbs, dtype=OBB_DTYPE)
        h = C.c_void_p()
        check(lib().epp_world_create(_ptr(obbs) if len(obbs) else None, len(obbs), r_gate, r_obst, C.byref(h)))
        self.handle = h.value
        self.n = len(obbs)

    def update(self, obbs: np.ndarray) -> None:
        obbs = np.ascontiguousarray(obbs, dtype=OBB_DTYPE)
        check(lib().epp_world_update(self.handle, _ptr(obbs) if len(obbs) else None, len(obbs)))
        self.n = len(obbs)

    def build_index(self) -> None:
        """Rebuild + upload a stale device index now (epp_world_build_index)."""
        check(lib().epp_world_build_index(self.handle))

    def generation(self) -> int:
        g = C.c_uint64(0)
        check(lib().epp_world_generation(self.handle, C.byref(g)))
        return g.value

    def aabbs(self) -> np.ndarray:
        out = np.zeros((max(self.n, 1), 6))
        check(lib().epp_world_get_aabbs(self.handle, _ptr(out)))
        return out[: self.n]

    def close(self) -> None:
        if self.handle:
            lib().epp_world_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- device-pointer calls ----------------------------------------------------
    def check_states_dev(self, xyz_ptr, n, can_pass_gate, valid_ptr, compact_ptr=None, nvalid_ptr=None,
                         stream=None):
        check(lib().epp_check_states(self.handle, xyz_ptr, n, int(can_pass_gate), valid_ptr, compact_ptr,
                                     nvalid_ptr, stream))

    def check_motions_dev(self, s1_ptr, s2_ptr, n, can_pass_gate, mode, valid_ptr, stream=None):
        check(lib().epp_check_motions(self.handle, s1_ptr, s2_ptr, n, int(can_pass_gate), int(mode),
                                      valid_ptr, stream))

    # ---- host-array convenience (copies in/out) ----------------------------------
    def check_states(self, xyz: np.ndarray, can_pass_gate: bool = False, compact: bool = False):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        n = len(xyz)
        d_xyz = DeviceBuffer.from_array(xyz)
        d_valid = DeviceBuffer(n)
        if compact:
            d_idx = DeviceBuffer(4 * max(n, 1))
            d_cnt = DeviceBuffer(8)
            d_cnt.zero()
            self.check_states_dev(d_xyz.ptr, n, can_pass_gate, d_valid.ptr, d_idx.ptr, d_cnt.ptr)
            sync()
            cnt = int(d_cnt.download(np.int64, 1)[0])
            return d_valid.download(np.uint8, n), d_idx.download(np.int32, cnt)
        self.check_states_dev(d_xyz.ptr, n, can_pass_gate, d_valid.ptr)
        sync()
        return d_valid.download(np.uint8, n)

    def check_states_mindist(self, xyz: np.ndarray, min_distance: float) -> np.ndarray:
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        n = len(xyz)
        d_xyz = DeviceBuffer.from_array(xyz)
        d_valid = DeviceBuffer(n)
        check(lib().epp_check_states_mindist(self.handle, d_xyz.ptr, n, float(min_distance), d_valid.ptr, None))
        sync()
        return d_valid.download(np.uint8, n)

    def check_motions(self, s1: np.ndarray, s2: np.ndarray, can_pass_gate: bool = False, mode: int = 0):
        s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 3)
        s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 3)
        n = len(s1)
        d1, d2 = DeviceBuffer.from_array(s1), DeviceBuffer.from_array(s2)
        d_valid = DeviceBuffer(n)
        self.check_motions_dev(d1.ptr, d2.ptr, n, can_pass_gate, mode, d_valid.ptr)
        sync()
        return d_valid.download(np.uint8, n)

    def check_trajectories(self, Ts, Cs, dt: float, min_distance: float):
        """epp_traj_check_batch on the lists minsnap_batch returns: per track the index of the
        first sampled row (Trajectory::evaluateRange at dt) closer than min_distance to an OBB
        and its time, (-1, -1.0) for a collision-free track.  Returns (int64[n], float64[n])."""
        nt = len(Ts)
        d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
        d_row, d_time = DeviceBuffer(8 * nt), DeviceBuffer(8 * nt)
        check(lib().epp_traj_check_batch(self.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, float(dt), float(min_distance),
                                         d_row.ptr, d_time.ptr, None))
        sync()
        return d_row.download(np.int64, nt), d_time.download(np.float64, nt)

    def sweep_trajectories(self, Ts, Cs, dt: float, can_pass_gate: bool = False):
        """epp_traj_sweep_batch on the lists minsnap_batch returns: per track the index j of the
        first chord row j -> row j + 1 (rows of Trajectory::evaluateRange at dt) that fails
        World::checkRayValid and row j's time, (-1, -1.0) when no chord fails.  Returns
        (int64[n], float64[n])."""
        nt = len(Ts)
        d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
        d_row, d_time = DeviceBuffer(8 * nt), DeviceBuffer(8 * nt)
        check(lib().epp_traj_sweep_batch(self.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, float(dt),
                                         1 if can_pass_gate else 0, d_row.ptr, d_time.ptr, None))
        sync()
        return d_row.download(np.int64, nt), d_time.download(np.float64, nt)

    def clearance(self, points: np.ndarray):
        """epp_states_clearance: per point the Euclidean distance to the nearest collision
        (non-filling) OBB, 0 inside or on one, and that OBB's index in the world's order (the
        lowest index among equals); (+inf, -1) without a collision OBB or for a non-finite
        point.  Returns (float64[n], int32[n])."""
        xyz = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        n = len(xyz)
        d_xyz = DeviceBuffer.from_array(xyz)
        d_dist, d_near = DeviceBuffer(8 * n), DeviceBuffer(4 * n)
        check(lib().epp_states_clearance(self.handle, d_xyz.ptr, n, d_dist.ptr, d_near.ptr, None))
        sync()
        return d_dist.download(np.float64, n), d_near.download(np.int32, n)

    def trajectory_clearance(self, Ts, Cs, dt: float):
        """epp_traj_clearance_batch on the lists minsnap_batch returns: per track the closest
        approach of its sampled rows (Trajectory::evaluateRange at dt) to a collision OBB, the
        earliest row that attains it, that row's time and its nearest OBB; (+inf, -1, -1.0, -1)
        for a track without rows or a world without collision OBBs.  Returns (float64[n],
        int64[n], float64[n], int32[n])."""
        nt = len(Ts)
        d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
        d_clr, d_row, d_time, d_near = (DeviceBuffer(8 * nt), DeviceBuffer(8 * nt), DeviceBuffer(8 * nt),
                                        DeviceBuffer(4 * nt))
        check(lib().epp_traj_clearance_batch(self.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, float(dt), d_clr.ptr,
                                             d_row.ptr, d_time.ptr, d_near.ptr, None))
        sync()
        return (d_clr.download(np.float64, nt), d_row.download(np.int64, nt), d_time.download(np.float64, nt),
                d_near.download(np.int32, nt))

    def edge_clearances(self, s1: np.ndarray, s2: np.ndarray):
        """epp_motions_clearance: per edge s1[i] -> s2[i] the Euclidean distance between the
        segment and the nearest collision (non-filling) OBB, 0 for an edge that touches or
        enters one, the parameter in [0, 1] at which the edge is that close and that OBB's
        index in the world's order (the lowest index among equals); (+inf, -1.0, -1) without a
        collision OBB or for an edge with a non-finite coordinate.  Returns (float64[n],
        float64[n], int32[n])."""
        s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 3)
        s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 3)
        n = len(s1)
        assert len(s2) == n
        d1, d2 = DeviceBuffer.from_array(s1), DeviceBuffer.from_array(s2)
        d_dist, d_t, d_near = DeviceBuffer(8 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n)
        check(lib().epp_motions_clearance(self.handle, d1.ptr, d2.ptr, n, d_dist.ptr, d_t.ptr, d_near.ptr, None))
        sync()
        return d_dist.download(np.float64, n), d_t.download(np.float64, n), d_near.download(np.int32, n)

    def trajectory_chord_clearances(self, Ts, Cs, dt: float):
        """epp_traj_chord_clearance_batch on the lists minsnap_batch returns: per track the
        closest approach of the straight chords between its consecutive sampled rows
        (Trajectory::evaluateRange at dt) to a collision OBB, the earliest chord that attains
        it, the parameter along that chord, the track time of that point and the nearest OBB;
        (+inf, -1, -1.0, -1.0, -1) for a track with fewer than two rows or a world without
        collision OBBs.  Returns (float64[n], int64[n], float64[n], float64[n], int32[n])."""
        nt = len(Ts)
        d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
        d_clr, d_chord, d_t, d_time, d_near = (DeviceBuffer(8 * nt), DeviceBuffer(8 * nt), DeviceBuffer(8 * nt),
                                               DeviceBuffer(8 * nt), DeviceBuffer(4 * nt))
        check(lib().epp_traj_chord_clearance_batch(self.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, float(dt), d_clr.ptr,
                                                   d_chord.ptr, d_t.ptr, d_time.ptr, d_near.ptr, None))
        sync()
        return (d_clr.download(np.float64, nt), d_chord.download(np.int64, nt), d_t.download(np.float64, nt),
                d_time.download(np.float64, nt), d_near.download(np.int32, nt))

    def first_hits(self, s1: np.ndarray, s2: np.ndarray, can_pass_gate: bool = False):
        """epp_motions_first_hit: per edge s1[i] -> s2[i] the parameter in [0, 1] at which it
        first enters an OBB that World::checkRayValid rejects it for (0: the start is in
        collision) and that OBB's index in the world's order (the lowest index among equals);
        (+inf, -1) for an edge check_motions (mode 0) calls valid.  Returns (float64[n],
        int32[n])."""
        s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 3)
        s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 3)
        n = len(s1)
        assert len(s2) == n
        d1, d2 = DeviceBuffer.from_array(s1), DeviceBuffer.from_array(s2)
        d_t, d_obb = DeviceBuffer(8 * n), DeviceBuffer(4 * n)
        check(lib().epp_motions_first_hit(self.handle, d1.ptr, d2.ptr, n, 1 if can_pass_gate else 0, d_t.ptr,
                                          d_obb.ptr, None))
        sync()
        return d_t.download(np.float64, n), d_obb.download(np.int32, n)

    def trajectory_first_hits(self, Ts, Cs, dt: float, can_pass_gate: bool = False):
        """epp_traj_first_hit_batch on the lists minsnap_batch returns: per track the first
        failing chord (sweep_trajectories' answer), the parameter along it at which it enters
        the blocking OBB, the track time of that point and the OBB; (-1, +inf, -1.0, -1) when
        no chord fails.  Returns (int64[n], float64[n], float64[n], int32[n])."""
        nt = len(Ts)
        d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
        d_chord, d_t, d_time, d_obb = (DeviceBuffer(8 * nt), DeviceBuffer(8 * nt), DeviceBuffer(8 * nt),
                                       DeviceBuffer(4 * nt))
        check(lib().epp_traj_first_hit_batch(self.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, float(dt),
                                             1 if can_pass_gate else 0, d_chord.ptr, d_t.ptr, d_time.ptr, d_obb.ptr,
                                             None))
        sync()
        return (d_chord.download(np.int64, nt), d_t.download(np.float64, nt), d_time.download(np.float64, nt),
                d_obb.download(np.int32, nt))


def _take_rows(rows, n, cols=10) -> np.ndarray:
    """The n rows a *_host call handed out as an (n, cols) array of its own; the call's buffer is
    freed (epp_host_free)."""
    out = np.ctypeslib.as_array(rows, shape=(n.value * cols,)).copy().reshape(-1, cols) if n.value \
        else np.zeros((0, cols))
    lib().epp_host_free(C.cast(rows, C.c_void_p))
    return out


def _pack_waypoints(tracks):
    """A list of (W_k x 3) waypoint arrays as the batch calls take it: (wp float64[sum W_k, 3],
    off int32[n + 1], n, the number of segments sum W_k - n)."""
    tracks = [np.asarray(t, np.float64).reshape(-1, 3) for t in tracks]
    wp = np.ascontiguousarray(np.concatenate(tracks))
    off = np.zeros(len(tracks) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in tracks])
    return wp, off, len(tracks), int(off[-1]) - len(tracks)


def _split_tracks(T, Cf, off):
    """The per-segment arrays T and Cf (either may be None) of a batch with waypoint offsets off
    as per-track lists: track k's segments are off[k] - k .. off[k + 1] - k - 2."""
    spans = [(int(off[k]) - k, max(int(off[k]) - k, int(off[k + 1]) - k - 1)) for k in range(len(off) - 1)]
    return tuple(None if a is None else [a[i:j] for i, j in spans] for a in (T, Cf))


def minsnap_batch(tracks, v_max, a_max, v0=None, a0=None):
    """epp_minsnap_batch on a list of (W_k x 3) waypoint arrays.

    Returns (seg_times list, coeffs list [M_k x 3 x 10], status array)."""
    wp, off, nt, nseg = _pack_waypoints(tracks)
    d_wp, d_off = DeviceBuffer.from_array(wp), DeviceBuffer.from_array(off)
    d_v0 = DeviceBuffer.from_array(np.ascontiguousarray(v0, np.float64)) if v0 is not None else None
    d_a0 = DeviceBuffer.from_array(np.ascontiguousarray(a0, np.float64)) if a0 is not None else None
    d_T, d_C, d_st = DeviceBuffer(8 * max(nseg, 1)), DeviceBuffer(240 * max(nseg, 1)), DeviceBuffer(4 * nt)
    check(lib().epp_minsnap_batch(d_wp.ptr, d_off.ptr, nt, float(v_max), float(a_max),
                                  d_v0.ptr if d_v0 else None, d_a0.ptr if d_a0 else None,
                                  d_T.ptr, d_C.ptr, d_st.ptr, None))
    sync()
    T = d_T.download(np.float64, nseg)
    Cf = d_C.download(np.float64, nseg * 30).reshape(nseg, 3, 10)
    st = d_st.download(np.int32, nt)
    Ts, Cs = _split_tracks(T, Cf, off)
    return Ts, Cs, st


def minsnap_batch_times(tracks, times, v0=None, a0=None):
    """epp_minsnap_batch_times: as minsnap_batch with the caller's segment times (a list
    of (W_k - 1) arrays; setupFromVertices(vertices, segment_times)).  Returns (coeffs
    list, status array)."""
    wp, off, nt, nseg = _pack_waypoints(tracks)
    T = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float64).ravel() for t in times]))
    assert len(T) == nseg
    d_wp, d_off, d_T = DeviceBuffer.from_array(wp), DeviceBuffer.from_array(off), DeviceBuffer.from_array(T)
    d_v0 = DeviceBuffer.from_array(np.ascontiguousarray(v0, np.float64)) if v0 is not None else None
    d_a0 = DeviceBuffer.from_array(np.ascontiguousarray(a0, np.float64)) if a0 is not None else None
    d_C, d_st = DeviceBuffer(240 * max(nseg, 1)), DeviceBuffer(4 * nt)
    check(lib().epp_minsnap_batch_times(d_wp.ptr, d_off.ptr, nt, d_v0.ptr if d_v0 else None,
                                        d_a0.ptr if d_a0 else None, d_T.ptr, d_C.ptr, d_st.ptr, None))
    sync()
    Cf = d_C.download(np.float64, nseg * 30).reshape(nseg, 3, 10)
    st = d_st.download(np.int32, nt)
    return _split_tracks(None, Cf, off)[1], st


def minsnap_batch_constrained(tracks, v_max, a_max, masks, values, times=None):
    """epp_minsnap_batch_constrained on a list of (W_k x 3) waypoint arrays: masks a list of
    uint8[W_k] (bit k-1: derivative k is fixed at the waypoint; ignored at a track's two ends,
    where all four are), values a list of float64[W_k, 4, 3] (derivative k at [w, k-1]; slots
    whose bit is clear at inner waypoints are not read), times a list of (W_k - 1) segment
    times or None (Nfabian times under v_max / a_max, which ignore the fixed values).

    Returns (seg_times list, coeffs list [M_k x 3 x 10], status array) like minsnap_batch."""
    nt = len(tracks)
    if nt == 0:
        check(lib().epp_minsnap_batch_constrained(None, None, 0, float(v_max), float(a_max), None, None, None,
                                                  None, None, None, None))
        return [], [], np.zeros(0, np.int32)
    wp, off, nt, nseg = _pack_waypoints(tracks)
    nw = len(wp)
    mask = np.ascontiguousarray(np.concatenate([np.asarray(m, np.uint8).ravel() for m in masks]))
    val = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).reshape(-1, 12) for v in values]))
    if len(mask) != nw or len(val) != nw:
        raise ValueError("minsnap_batch_constrained: masks and values need one entry per waypoint")
    d_wp, d_off = DeviceBuffer.from_array(wp), DeviceBuffer.from_array(off)
    d_mask, d_val = DeviceBuffer.from_array(mask), DeviceBuffer.from_array(val)
    d_Tin = None
    if times is not None:
        Tin = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float64).ravel() for t in times] + [np.zeros(0)]))
        if len(Tin) != nseg:
            raise ValueError("minsnap_batch_constrained: times needs one entry per segment")
        d_Tin = DeviceBuffer.from_array(Tin) if nseg else DeviceBuffer(8)
    d_T, d_C, d_st = DeviceBuffer(8 * max(nseg, 1)), DeviceBuffer(240 * max(nseg, 1)), DeviceBuffer(4 * nt)
    d_T.zero()
    d_C.zero()
    check(lib().epp_minsnap_batch_constrained(d_wp.ptr, d_off.ptr, nt, float(v_max), float(a_max),
                                              d_Tin.ptr if d_Tin else None, d_mask.ptr, d_val.ptr, d_T.ptr, d_C.ptr,
                                              d_st.ptr, None))
    sync()
    T = d_T.download(np.float64, nseg)
    Cf = d_C.download(np.float64, nseg * 30).reshape(nseg, 3, 10)
    st = d_st.download(np.int32, nt)
    Ts, Cs = _split_tracks(T, Cf, off)
    return Ts, Cs, st


def generate_trajectory_constrained(waypoints, v_max, a_max, dt, mask, values, seg_times=None, t0=0.0) -> np.ndarray:
    """generateTrajectory under the caller's constraints (epp_generate_trajectory_constrained_host):
    mask uint8[W], values float64[W, 4, 3] as in minsnap_batch_constrained; seg_times None: Nfabian."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    mask = np.ascontiguousarray(np.asarray(mask, np.uint8).ravel())
    val = np.ascontiguousarray(np.asarray(values, np.float64).reshape(-1, 12))
    if len(mask) != len(wp) or len(val) != len(wp):
        raise ValueError("generate_trajectory_constrained: mask and values need one entry per waypoint")
    T = None if seg_times is None else np.ascontiguousarray(seg_times, np.float64)
    if T is not None and len(T) != len(wp) - 1:
        raise ValueError("generate_trajectory_constrained: seg_times needs one entry per segment")
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    check(lib().epp_generate_trajectory_constrained_host(_ptr(wp), len(wp), float(v_max), float(a_max),
                                                         _ptr(T) if T is not None else None, float(dt), float(t0),
                                                         _ptr(mask), _ptr(val), C.byref(rows), C.byref(n)))
    return _take_rows(rows, n)


def generate_trajectory_times(waypoints, seg_times, dt, t0=0.0, v0=(0, 0, 0), a0=(0, 0, 0)) -> np.ndarray:
    """generateTrajectory with the caller's segment times (epp_generate_trajectory_times_host)."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    T = np.ascontiguousarray(seg_times, np.float64)
    v0 = np.ascontiguousarray(v0, np.float64)
    a0 = np.ascontiguousarray(a0, np.float64)
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    check(lib().epp_generate_trajectory_times_host(_ptr(wp), len(wp), _ptr(T), float(dt), float(t0), _ptr(v0),
                                                   _ptr(a0), C.byref(rows), C.byref(n)))
    return _take_rows(rows, n)


def generate_trajectory(waypoints, v_max, a_max, dt, t0=0.0, v0=(0, 0, 0), a0=(0, 0, 0)) -> np.ndarray:
    """poly_traj::generateTrajectory (src/trajectory_generator.cpp:12-100) on the GPU."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    v0 = np.ascontiguousarray(v0, np.float64)
    a0 = np.ascontiguousarray(a0, np.float64)
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    check(lib().epp_generate_trajectory_host(_ptr(wp), len(wp), float(v_max), float(a_max), float(dt), float(t0),
                                             _ptr(v0), _ptr(a0), C.byref(rows), C.byref(n)))
    return _take_rows(rows, n)


def _upload_tracks(Ts, Cs):
    """The device layout of epp_minsnap_batch's outputs for lists of per-track segment times
    and coefficients (a track of W waypoints has W - 1 segments; an empty entry stands for a
    1-waypoint track)."""
    Ts = [np.asarray(t, np.float64).ravel() for t in Ts]
    nt = len(Ts)
    off = np.zeros(nt + 1, np.int32)
    off[1:] = np.cumsum([len(t) + 1 for t in Ts])
    nseg = int(sum(len(t) for t in Ts))
    T = np.concatenate(Ts + [np.zeros(0)])
    Cf = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3, 10) for c in Cs] + [np.zeros((0, 3, 10))])
    assert len(Cf) == nseg
    d_T, d_C = DeviceBuffer(8 * max(nseg, 1)), DeviceBuffer(240 * max(nseg, 1))
    if nseg:
        d_T.upload(T)
        d_C.upload(Cf)
    return d_T, d_C, DeviceBuffer.from_array(off), off, nseg


def sample_count(Ts, dt: float) -> np.ndarray:
    """epp_sample_count on the segment-time lists minsnap_batch returns: the number of rows
    Trajectory::evaluateRange(0, max_time, dt) gives per track.  Returns int64[n]."""
    nt = len(Ts)
    if nt == 0:
        return np.zeros(0, np.int64)
    Ts = [np.asarray(t, np.float64).ravel() for t in Ts]
    off = np.zeros(nt + 1, np.int32)
    off[1:] = np.cumsum([len(t) + 1 for t in Ts])
    d_T, d_off = DeviceBuffer.from_array(np.concatenate(Ts + [np.zeros(1)])), DeviceBuffer.from_array(off)
    d_cnt = DeviceBuffer(8 * nt)
    check(lib().epp_sample_count(d_T.ptr, d_off.ptr, nt, float(dt), d_cnt.ptr, None))
    sync()
    return d_cnt.download(np.int64, nt)


def sample_batch(Ts, Cs, dt: float, t0=None, row_offsets=None, n_rows=None, fill=None) -> np.ndarray:
    """epp_sample_batch on the lists minsnap_batch returns: the rows [x, vx, ax, y, vy, ay, z,
    vz, az, t] of every track, track k's time column offset by t0[k] (None: the call's NULL).

    By default the tracks' rows follow each other (the exclusive scan of sample_count) and the
    buffer holds exactly them.  row_offsets (int64[n], track k's first row) with n_rows (the
    buffer's size in rows): the caller lays the tracks out; every track's range must lie inside
    the buffer (checked here against sample_count, before the launch).  fill: the float64 bit
    pattern (a u64) every slot of the buffer holds before the launch, None: zeros.
    Returns float64[n_rows, 10]."""
    nt = len(Ts)
    dt = float(dt)
    d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
    cnt = np.zeros(nt, np.int64)
    if nt:
        d_cnt = DeviceBuffer(8 * nt)
        check(lib().epp_sample_count(d_T.ptr, d_off.ptr, nt, dt, d_cnt.ptr, None))
        sync()
        cnt = d_cnt.download(np.int64, nt)
    if row_offsets is None:
        if n_rows is not None:
            raise ValueError("sample_batch: n_rows goes with row_offsets")
        roff = np.zeros(nt, np.int64)
        roff[1:] = np.cumsum(cnt)[:-1]
        n_rows = int(cnt.sum())
    else:
        roff = np.ascontiguousarray(row_offsets, np.int64).reshape(-1)
        if n_rows is None or len(roff) != nt:
            raise ValueError("sample_batch: row_offsets needs one entry per track and n_rows")
        n_rows = int(n_rows)
        if n_rows < 0 or (roff < 0).any() or (roff + cnt > n_rows).any():
            raise ValueError("sample_batch: a track's rows do not fit the buffer")
    d_rows = _filled(80 * max(n_rows, 1), fill)
    if nt:
        d_t0 = None
        if t0 is not None:
            t0 = np.ascontiguousarray(t0, np.float64).reshape(-1)
            if len(t0) != nt:
                raise ValueError("sample_batch: t0 needs one entry per track")
            d_t0 = DeviceBuffer.from_array(t0)
        d_roff = DeviceBuffer.from_array(roff)
        check(lib().epp_sample_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, d_t0.ptr if d_t0 else None, d_roff.ptr,
                                     d_rows.ptr, None))
        sync()
    return d_rows.download(np.float64, n_rows * 10).reshape(n_rows, 10)


GATE_HALF_EDGE = 0.425  # OnlineTrajGenerator::checkGatePassed's edgeLength (src/OnlineTrajGenerator.cpp:249)


def gate_frames(centres, yaws) -> np.ndarray:
    """The gate frame table of gates_crossed / trajectory_gate_passes: (G, 5) rows
    [cx, cy, cz, cos(yaw), sin(yaw)] from the gate centres (G, 3) and yaws (G), with numpy's
    cos / sin.  (PathPlanner.gate_frames builds it from gate rows and the config's heights.)"""
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    yaws = np.asarray(yaws, np.float64).reshape(-1)
    assert len(yaws) == len(centres)
    return np.ascontiguousarray(np.column_stack([centres, np.cos(yaws), np.sin(yaws)]))


def gate_velocity_pins(frames, waypoints, gate_rows, speed: float):
    """The constraints that send one track through its gates along their normals: for every
    inner waypoint w with gate_rows[w] = g >= 0 (the row of the frame table whose centre the
    waypoint sits at; -1: no gate), derivative 1 is fixed to speed times gate g's normal.  The
    normal is the gate frame's y axis, (sin(yaw), cos(yaw), 0) in the world (gate_pass.h: a
    crossing goes from negative to positive gate-frame y), with the sign that gives it a
    non-negative dot product with (next waypoint - previous waypoint).  The first and the last
    waypoint are left alone: their states are the caller's.  Host code only.

    Returns (mask uint8[W], values float64[W, 4, 3]) for minsnap_batch_constrained, the two end
    rows of values zero."""
    frames = np.asarray(frames, np.float64).reshape(-1, 5)
    wp = np.asarray(waypoints, np.float64).reshape(-1, 3)
    rows = np.asarray(gate_rows, np.int64).reshape(-1)
    if len(rows) != len(wp):
        raise ValueError("gate_velocity_pins: gate_rows needs one entry per waypoint")
    if (rows >= len(frames)).any():
        raise ValueError("gate_velocity_pins: a gate row is outside the frame table")
    mask = np.zeros(len(wp), np.uint8)
    values = np.zeros((len(wp), 4, 3))
    for w in range(1, len(wp) - 1):
        g = int(rows[w])
        if g < 0:
            continue
        n = np.array([frames[g, 4], frames[g, 3], 0.0])
        if np.dot(n, wp[w + 1] - wp[w - 1]) < 0.0:
            n = -n
        mask[w] |= 1
        values[w, 0] = float(speed) * n
    return mask, values


def gates_crossed(frames, half_edge: float, s1: np.ndarray, s2: np.ndarray) -> np.ndarray:
    """epp_gates_crossed: per edge s1[i] -> s2[i] a uint64 whose bit g says that the edge
    crosses gate g of the frame table (at most 64 gates) from its negative to its positive
    side within half_edge of its centre (checkGatePassed).  Returns uint64[n]."""
    frames = np.ascontiguousarray(frames, np.float64).reshape(-1, 5)
    s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 3)
    s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 3)
    n = len(s1)
    assert len(s2) == n
    d_f, d1, d2 = DeviceBuffer.from_array(frames), DeviceBuffer.from_array(s1), DeviceBuffer.from_array(s2)
    d_m = DeviceBuffer(8 * n)
    check(lib().epp_gates_crossed(d_f.ptr, len(frames), float(half_edge), d1.ptr, d2.ptr, n, d_m.ptr, None))
    sync()
    return d_m.download(np.uint64, n)


def trajectory_gate_passes(frames, half_edge: float, Ts, Cs, dt: float):
    """epp_traj_gate_pass_batch on the lists minsnap_batch returns: per track and gate the
    chord row j -> row j + 1 that passes the gate after the gates before it (-1: unpassed),
    its split time (-1.0) and the crossing's midpoint offsets in the gate frame (NaN), and per
    track the number of leading gates passed.  Returns (int64[n, G], float64[n, G],
    float64[n, G, 2], int32[n])."""
    frames = np.ascontiguousarray(frames, np.float64).reshape(-1, 5)
    nt, G = len(Ts), len(frames)
    d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
    d_f = DeviceBuffer.from_array(frames)
    d_chord, d_time, d_o, d_np = (DeviceBuffer(8 * nt * G), DeviceBuffer(8 * nt * G), DeviceBuffer(16 * nt * G),
                                  DeviceBuffer(4 * nt))
    check(lib().epp_traj_gate_pass_batch(d_f.ptr, G, float(half_edge), d_T.ptr, d_C.ptr, d_off.ptr, nt, float(dt),
                                         d_chord.ptr, d_time.ptr, d_o.ptr, d_np.ptr, None))
    sync()
    return (d_chord.download(np.int64, nt * G).reshape(nt, G), d_time.download(np.float64, nt * G).reshape(nt, G),
            d_o.download(np.float64, nt * G * 2).reshape(nt, G, 2), d_np.download(np.int32, nt))


GRAVITY = 9.81  # m/s^2: the default g of thrust_rates / trajectory_thrust_rates


def sample_derivative(Ts, Cs, dt: float, order: int):
    """epp_sample_derivative_batch on the lists minsnap_batch returns: derivative `order`
    (0..9) of every row of every track, [x, y, z]; the tracks' rows follow each other (the
    exclusive scan of sample_count).  Returns (float64[n_rows, 3], int64[n + 1] row offsets)."""
    nt = len(Ts)
    dt = float(dt)
    d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
    roff = np.zeros(nt + 1, np.int64)
    if nt:
        d_cnt = DeviceBuffer(8 * nt)
        check(lib().epp_sample_count(d_T.ptr, d_off.ptr, nt, dt, d_cnt.ptr, None))
        sync()
        roff[1:] = np.cumsum(d_cnt.download(np.int64, nt))
    n_rows = int(roff[-1])
    d_val = _filled(24 * max(n_rows, 1), None)
    d_roff = DeviceBuffer.from_array(roff)
    check(lib().epp_sample_derivative_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, int(order), d_roff.ptr, d_val.ptr,
                                            None))
    sync()
    return d_val.download(np.float64, n_rows * 3).reshape(n_rows, 3), roff


def thrust_rates(acc, jerk, g: float = GRAVITY):
    """epp_thrust_rates: per sample, from its acceleration and jerk (n x 3 each), the
    mass-normalised thrust |a + g e_z|, the roll / pitch body rate |F x j| / |F|^2 and the
    cosine of the tilt F_z / |F|.  Returns (float64[n], float64[n], float64[n])."""
    acc = np.ascontiguousarray(acc, np.float64).reshape(-1, 3)
    jerk = np.ascontiguousarray(jerk, np.float64).reshape(-1, 3)
    n = len(acc)
    assert len(jerk) == n
    d_a, d_j = DeviceBuffer.from_array(acc), DeviceBuffer.from_array(jerk)
    d_f, d_r, d_c = DeviceBuffer(8 * n), DeviceBuffer(8 * n), DeviceBuffer(8 * n)
    check(lib().epp_thrust_rates(d_a.ptr, d_j.ptr, n, float(g), d_f.ptr, d_r.ptr, d_c.ptr, None))
    sync()
    return d_f.download(np.float64, n), d_r.download(np.float64, n), d_c.download(np.float64, n)


def trajectory_thrust_rates(Ts, Cs, dt: float, g: float = GRAVITY):
    """epp_traj_thrust_rates_batch on the lists minsnap_batch returns: per track [f_min,
    t_fmin, f_max, t_fmax, rate_max, t_rate, cos_min, t_cos] over its rows at dt and the four
    rows that attain them (-1: none).  Returns (float64[n, 8], int64[n, 4])."""
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
    d_out, d_rows = DeviceBuffer(64 * nt), DeviceBuffer(32 * nt)
    check(lib().epp_traj_thrust_rates_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, float(dt), float(g), d_out.ptr,
                                            d_rows.ptr, None))
    sync()
    return d_out.download(np.float64, 8 * nt).reshape(nt, 8), d_rows.download(np.int64, 4 * nt).reshape(nt, 4)


def traj_peaks(Ts, Cs):
    """epp_traj_peaks on the lists minsnap_batch returns: ((n, 4) array [v_peak, t_v, a_peak,
    t_a], status array)."""
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
    d_pk, d_st = DeviceBuffer(32 * nt), DeviceBuffer(4 * nt)
    check(lib().epp_traj_peaks(d_T.ptr, d_C.ptr, d_off.ptr, nt, d_pk.ptr, d_st.ptr, None))
    sync()
    return d_pk.download(np.float64, 4 * nt).reshape(nt, 4), d_st.download(np.int32, nt)


def scale_to_limits(Ts, Cs, v_max, a_max):
    """epp_traj_scale_to_limits: (new seg_times list, new coeffs list, scale array, status array)."""
    nt = len(Ts)
    d_T, d_C, d_off, off, nseg = _upload_tracks(Ts, Cs)
    d_sc, d_st = DeviceBuffer(8 * nt), DeviceBuffer(4 * nt)
    check(lib().epp_traj_scale_to_limits(d_T.ptr, d_C.ptr, d_off.ptr, nt, float(v_max), float(a_max), d_sc.ptr,
                                         d_st.ptr, None))
    sync()
    T = d_T.download(np.float64, nseg)
    Cf = d_C.download(np.float64, nseg * 30).reshape(nseg, 3, 10)
    Tn, Cn = _split_tracks(T, Cf, off)
    return Tn, Cn, d_sc.download(np.float64, nt), d_st.download(np.int32, nt)


def generate_trajectory_limited(waypoints, v_max, a_max, dt, t0=0.0, v0=(0, 0, 0), a0=(0, 0, 0), return_scale=False):
    """epp_generate_trajectory_limited_host: generate_trajectory with the fit time-scaled to
    meet v_max / a_max (Trajectory::scaleSegmentTimesToMeetConstraints,
    external/poly_traj/src/trajectory.cpp:385-429).  return_scale: (rows, scale)."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    v0 = np.ascontiguousarray(v0, np.float64)
    a0 = np.ascontiguousarray(a0, np.float64)
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    scale = C.c_double(1.0)
    check(lib().epp_generate_trajectory_limited_host(_ptr(wp), len(wp), float(v_max), float(a_max), float(dt),
                                                     float(t0), _ptr(v0), _ptr(a0), C.byref(rows), C.byref(n),
                                                     C.byref(scale)))
    out = _take_rows(rows, n)
    return (out, scale.value) if return_scale else out


def thrust_grid(Ts, Cs, g: float = GRAVITY, scale=None):
    """epp_traj_thrust_grid_batch on the lists minsnap_batch returns: per track [f_min, t_fmin,
    f_max, t_fmax, rate_max, t_rate, cos_min, t_cos] over the 65 grid points of every segment
    at the per-track scale (None: 1), times in the input track's time.  Returns float64[n, 8]."""
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
    d_out = DeviceBuffer(64 * max(nt, 1))
    d_s = None
    if scale is not None:
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (nt,)))
        d_s = DeviceBuffer.from_array(sc if nt else np.zeros(1))
    check(lib().epp_traj_thrust_grid_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, d_s.ptr if d_s else None, float(g),
                                           d_out.ptr, None))
    sync()
    return d_out.download(np.float64, 8 * nt).reshape(nt, 8)


def scale_to_thrust_limits(Ts, Cs, g, f_min, f_max, rate_max, cos_tilt_min):
    """epp_traj_scale_to_thrust_limits: (new seg_times list, new coeffs list, scale array,
    status array, violated array)."""
    nt = len(Ts)
    d_T, d_C, d_off, off, nseg = _upload_tracks(Ts, Cs)
    d_sc, d_st, d_vi = DeviceBuffer(8 * max(nt, 1)), DeviceBuffer(4 * max(nt, 1)), DeviceBuffer(4 * max(nt, 1))
    check(lib().epp_traj_scale_to_thrust_limits(d_T.ptr, d_C.ptr, d_off.ptr, nt, float(g), float(f_min),
                                                float(f_max), float(rate_max), float(cos_tilt_min), d_sc.ptr,
                                                d_st.ptr, d_vi.ptr, None))
    sync()
    T = d_T.download(np.float64, nseg)
    Cf = d_C.download(np.float64, nseg * 30).reshape(nseg, 3, 10)
    Tn, Cn = _split_tracks(T, Cf, off)
    return Tn, Cn, d_sc.download(np.float64, nt), d_st.download(np.int32, nt), d_vi.download(np.int32, nt)


def snap_cost(Ts, Cs):
    """epp_traj_snap_cost on the lists minsnap_batch returns: (cost array, status array)."""
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = _upload_tracks(Ts, Cs)
    d_J, d_st = DeviceBuffer(8 * max(nt, 1)), DeviceBuffer(4 * max(nt, 1))
    check(lib().epp_traj_snap_cost(d_T.ptr, d_C.ptr, d_off.ptr, nt, d_J.ptr, d_st.ptr, None))
    sync()
    return d_J.download(np.float64, nt), d_st.download(np.int32, nt)


def _upload_fit_inputs(tracks, times, v0, a0):
    wp, off, _, nseg = _pack_waypoints(tracks)
    T = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float64).ravel() for t in times] + [np.zeros(0)]))
    assert len(T) == nseg
    d_wp, d_off = DeviceBuffer.from_array(wp), DeviceBuffer.from_array(off)
    d_T = DeviceBuffer.from_array(T if nseg else np.zeros(1))
    d_v0 = DeviceBuffer.from_array(np.ascontiguousarray(v0, np.float64)) if v0 is not None else None
    d_a0 = DeviceBuffer.from_array(np.ascontiguousarray(a0, np.float64)) if a0 is not None else None
    return d_wp, d_off, d_T, d_v0, d_a0, off, nseg


def time_gradient(tracks, times, h=0.1, t_min=0.1, v0=None, a0=None):
    """epp_minsnap_time_gradient: the snap cost of the fit at the caller's segment times (a list
    of (W_k - 1) arrays) and its Mellinger gradient.  Returns (cost array, grad list, status
    array)."""
    nt = len(tracks)
    d_wp, d_off, d_T, d_v0, d_a0, off, nseg = _upload_fit_inputs(tracks, times, v0, a0)
    d_J, d_g, d_st = DeviceBuffer(8 * nt), DeviceBuffer(8 * max(nseg, 1)), DeviceBuffer(4 * nt)
    check(lib().epp_minsnap_time_gradient(d_wp.ptr, d_off.ptr, nt, d_v0.ptr if d_v0 else None,
                                          d_a0.ptr if d_a0 else None, d_T.ptr, float(h), float(t_min), d_J.ptr,
                                          d_g.ptr, d_st.ptr, None))
    sync()
    g = d_g.download(np.float64, nseg)
    return d_J.download(np.float64, nt), _split_tracks(g, None, off)[0], d_st.download(np.int32, nt)


def optimize_times(tracks, times, params=None, v0=None, a0=None):
    """epp_minsnap_optimize_times from the caller's segment times.  params: a TimeoptParams
    (None: the defaults).  Returns (seg_times list, coeffs list, cost0, cost1, iters, status)."""
    nt = len(tracks)
    d_wp, d_off, d_T, d_v0, d_a0, off, nseg = _upload_fit_inputs(tracks, times, v0, a0)
    d_C = DeviceBuffer(240 * max(nseg, 1))
    d_C.zero()
    d_J0, d_J1, d_it, d_st = DeviceBuffer(8 * nt), DeviceBuffer(8 * nt), DeviceBuffer(4 * nt), DeviceBuffer(4 * nt)
    check(lib().epp_minsnap_optimize_times(d_wp.ptr, d_off.ptr, nt, d_v0.ptr if d_v0 else None,
                                           d_a0.ptr if d_a0 else None, d_T.ptr, d_C.ptr,
                                           params if params is not None else TimeoptParams(), d_J0.ptr, d_J1.ptr,
                                           d_it.ptr, d_st.ptr, None))
    sync()
    T = d_T.download(np.float64, nseg)
    Cf = d_C.download(np.float64, nseg * 30).reshape(nseg, 3, 10)
    Tn, Cn = _split_tracks(T, Cf, off)
    return (Tn, Cn, d_J0.download(np.float64, nt), d_J1.download(np.float64, nt), d_it.download(np.int32, nt),
            d_st.download(np.int32, nt))


def generate_trajectory_timeopt(waypoints, v_max, a_max, dt, params=None, t0=0.0, v0=(0, 0, 0), a0=(0, 0, 0),
                                enforce_va=False, limits=None, return_costs=False):
    """epp_generate_trajectory_timeopt_host: generate_trajectory with the segment times
    optimised (epp_minsnap_optimize_times under params, None: the defaults), then scaled to
    v_max / a_max when enforce_va and to limits = (g, f_min, f_max, rate_max, cos_tilt_min) when
    given.  return_costs: (rows, cost0, cost1, iters)."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    v0 = np.ascontiguousarray(v0, np.float64)
    a0 = np.ascontiguousarray(a0, np.float64)
    tl = np.ascontiguousarray(limits, np.float64) if limits is not None else None
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    j0, j1, it = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    check(lib().epp_generate_trajectory_timeopt_host(_ptr(wp), len(wp), float(v_max), float(a_max), float(dt),
                                                     float(t0), _ptr(v0), _ptr(a0),
                                                     params if params is not None else TimeoptParams(),
                                                     1 if enforce_va else 0, _ptr(tl) if tl is not None else None,
                                                     C.byref(rows), C.byref(n), C.byref(j0), C.byref(j1),
                                                     C.byref(it)))
    out = _take_rows(rows, n)
    return (out, j0.value, j1.value, it.value) if return_costs else out


def generate_trajectory_flyable(waypoints, v_max, a_max, dt, limits, t0=0.0, v0=(0, 0, 0), a0=(0, 0, 0),
                                enforce_va=False, return_scales=False):
    """epp_generate_trajectory_flyable_host: generate_trajectory with the fit time-scaled to
    meet v_max / a_max when enforce_va, then the thrust, body-rate and tilt limits
    limits = (g, f_min, f_max, rate_max, cos_tilt_min).  return_scales: (rows, scale_va,
    scale_thrust)."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    v0 = np.ascontiguousarray(v0, np.float64)
    a0 = np.ascontiguousarray(a0, np.float64)
    g, f_min, f_max, rate_max, cos_tilt_min = (float(x) for x in limits)
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    s_va, s_th = C.c_double(1.0), C.c_double(1.0)
    check(lib().epp_generate_trajectory_flyable_host(_ptr(wp), len(wp), float(v_max), float(a_max), float(dt),
                                                     float(t0), _ptr(v0), _ptr(a0), 1 if enforce_va else 0, g, f_min,
                                                     f_max, rate_max, cos_tilt_min, C.byref(rows), C.byref(n),
                                                     C.byref(s_va), C.byref(s_th)))
    out = _take_rows(rows, n)
    return (out, s_va.value, s_th.value) if return_scales else out


def check_and_generate_trajectory(world: "World", check_xyz, min_distance, waypoints, v_max, a_max, dt, t0=0.0,
                                  v0=(0, 0, 0), a0=(0, 0, 0)):
    """epp_check_and_generate_trajectory_host: (minDistance flags of check_xyz against the
    world, the trajectory rows of generate_trajectory) from one launch."""
    pts = np.ascontiguousarray(np.asarray(check_xyz, np.float64).reshape(-1, 3))
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    v0 = np.ascontiguousarray(v0, np.float64)
    a0 = np.ascontiguousarray(a0, np.float64)
    flags = np.zeros(max(len(pts), 1), np.uint8)
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    check(lib().epp_check_and_generate_trajectory_host(world.handle, _ptr(pts), len(pts), float(min_distance),
                                                       _ptr(flags), _ptr(wp), len(wp), float(v_max), float(a_max),
                                                       float(dt), float(t0), _ptr(v0), _ptr(a0), C.byref(rows),
                                                       C.byref(n)))
    out = _take_rows(rows, n)
    return flags[:len(pts)], out


def optimal_trajectory(waypoints, v_max, a_max, dt, t0=0.0, max_deviation=0.1, pre_waypoints=()) -> np.ndarray:
    """OptimalTimeParametrizer::calculateTrajectory (the "optimal" type; host code,
    external/time_parametrization/src/OptimalTimeParametrizer.cpp:11-108): rows x 11."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    pre = np.ascontiguousarray(np.asarray(pre_waypoints, np.float64).reshape(-1, 3))
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    check(lib().epp_optimal_trajectory_host(_ptr(wp), len(wp), _ptr(pre) if len(pre) else None, len(pre),
                                            float(v_max), float(a_max), float(dt), float(t0), float(max_deviation),
                                            C.byref(rows), C.byref(n)))
    return _take_rows(rows, n, 11)


def spline_trajectory(waypoints, max_t, dt, t0=0.0) -> np.ndarray:
    """TrajInterpolation::interpolateTraj (the "spline" type; host code,
    src/TrajInterpolation.cpp:44-68): rows x 10."""
    wp = np.ascontiguousarray(np.asarray(waypoints, np.float64).reshape(-1, 3))
    rows = C.POINTER(C.c_double)()
    n = C.c_int64(0)
    check(lib().epp_spline_trajectory_host(_ptr(wp), len(wp), float(max_t), float(t0), float(dt),
                                           C.byref(rows), C.byref(n)))
    return _take_rows(rows, n)


def sample_uniform(seed: int, lo, hi, n: int, start: int = 0) -> np.ndarray:
    """epp_sample_uniform: n counter-based uniform states (rows start..start+n-1)."""
    lo = np.ascontiguousarray(lo, np.float64)
    hi = np.ascontiguousarray(hi, np.float64)
    d = DeviceBuffer(24 * max(n, 1))
    check(lib().epp_sample_uniform(int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(lo), _ptr(hi), int(n), int(start), d.ptr, None))
    sync()
    return d.download(np.float64, 3 * n).reshape(n, 3)


def _filled(nbytes: int, word) -> DeviceBuffer:
    """A device buffer of nbytes (multiple of 8) holding `word` (u64) in every slot, or
    zeros when word is None -- a caller workspace that held other data."""
    b = DeviceBuffer(nbytes)
    if word is None:
        b.zero()
    else:
        b.upload(np.full(nbytes // 8, int(word) & 0xFFFFFFFFFFFFFFFF, np.uint64))
    return b


def knn(nodes: np.ndarray, k: int, max_dist: float = 0.0, method: str = "auto", box=None,
        ws_fill=None) -> np.ndarray:
    """epp_knn (method "auto"), epp_knn_bruteforce ("brute") or epp_knn_grid ("grid"):
    (n, k) neighbour indices, nearest first, ties to the lower index, -1 where fewer
    than k exist.  box=(lo, hi) with method "ws" / "grid_ws": the caller-box variants
    (epp_knn_ws_box / epp_knn_grid_ws_box; every node inside the box).  ws_fill: the u64
    word the caller workspace holds before the call (tests: stale data)."""
    nodes = np.ascontiguousarray(np.asarray(nodes, np.float64).reshape(-1, 3))
    n = len(nodes)
    d_n = DeviceBuffer.from_array(nodes)
    d_k = DeviceBuffer(4 * max(n * k, 1))
    if method in ("ws", "grid_ws"):  # caller workspace variants
        d_w = _filled(max(int(lib().epp_knn_workspace_size(n)), 256), ws_fill)
        if box is not None:
            lo, hi = (np.ascontiguousarray(np.asarray(b, np.float64).reshape(3)) for b in box)
            fn = lib().epp_knn_ws_box if method == "ws" else lib().epp_knn_grid_ws_box
            check(fn(d_n.ptr, n, int(k), float(max_dist), _ptr(lo), _ptr(hi), d_k.ptr, d_w.ptr, d_w.nbytes, None))
        else:
            fn = lib().epp_knn_ws if method == "ws" else lib().epp_knn_grid_ws
            check(fn(d_n.ptr, n, int(k), float(max_dist), d_k.ptr, d_w.ptr, d_w.nbytes, None))
    else:
        fn = {"auto": lib().epp_knn, "brute": lib().epp_knn_bruteforce, "grid": lib().epp_knn_grid}[method]
        check(fn(d_n.ptr, n, int(k), float(max_dist), d_k.ptr, None))
    sync()
    return d_k.download(np.int32, n * k).reshape(n, k)


def compact_states(xyz: np.ndarray, valid: np.ndarray, ws: bool = False, ws_fill=None) -> np.ndarray:
    """epp_compact_states (ws: epp_compact_states_ws, caller workspace): the valid rows of
    xyz, in index order.  ws_fill: the u64 word the caller workspace holds before the call."""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3))
    valid = np.ascontiguousarray(np.asarray(valid, np.uint8))
    n = len(xyz)
    d_x, d_v = DeviceBuffer.from_array(xyz), DeviceBuffer.from_array(valid)
    d_o, d_c = DeviceBuffer(24 * max(n, 1)), DeviceBuffer(8)
    if ws:
        d_w = _filled(int(lib().epp_compact_workspace_size(n)), ws_fill)
        check(lib().epp_compact_states_ws(d_x.ptr, d_v.ptr, n, d_o.ptr, d_c.ptr, d_w.ptr, d_w.nbytes, None))
    else:
        check(lib().epp_compact_states(d_x.ptr, d_v.ptr, n, d_o.ptr, d_c.ptr, None))
    sync()
    cnt = int(d_c.download(np.int64, 1)[0])
    return d_o.download(np.float64, 3 * cnt).reshape(cnt, 3) if cnt else np.zeros((0, 3))


def mask_edges(nbr: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """epp_mask_edges: nbr with -1 where valid == 0."""
    nbr = np.ascontiguousarray(np.asarray(nbr, np.int32))
    valid = np.ascontiguousarray(np.asarray(valid, np.uint8).reshape(nbr.shape))
    d_n, d_v = DeviceBuffer.from_array(nbr), DeviceBuffer.from_array(valid)
    check(lib().epp_mask_edges(d_n.ptr, d_v.ptr, nbr.size, None))
    sync()
    return d_n.download(np.int32, nbr.size).reshape(nbr.shape)


def mask_edges_count(nbr: np.ndarray, valid: np.ndarray, target: int = 1):
    """epp_mask_edges_count: (nbr with -1 where valid == 0, entries >= 0 afterwards,
    entries == target afterwards)."""
    nbr = np.ascontiguousarray(np.asarray(nbr, np.int32))
    valid = np.ascontiguousarray(np.asarray(valid, np.uint8).reshape(nbr.shape))
    d_n, d_v, d_c = DeviceBuffer.from_array(nbr), DeviceBuffer.from_array(valid), DeviceBuffer(16)
    check(lib().epp_mask_edges_count(d_n.ptr, d_v.ptr, nbr.size, target, d_c.ptr, None))
    sync()
    c = d_c.download(np.int64, 2)
    return d_n.download(np.int32, nbr.size).reshape(nbr.shape), int(c[0]), int(c[1])


def knn_edges(nodes: np.ndarray, nbr: np.ndarray):
    """epp_knn_edges: the (node, neighbour) endpoint arrays of every k-NN edge."""
    nodes = np.ascontiguousarray(np.asarray(nodes, np.float64).reshape(-1, 3))
    nbr = np.ascontiguousarray(nbr, np.int32)
    n, k = nbr.shape
    d_n, d_k = DeviceBuffer.from_array(nodes), DeviceBuffer.from_array(nbr)
    d_1, d_2 = DeviceBuffer(24 * max(n * k, 1)), DeviceBuffer(24 * max(n * k, 1))
    check(lib().epp_knn_edges(d_n.ptr, d_k.ptr, n, k, d_1.ptr, d_2.ptr, None))
    sync()
    return d_1.download(np.float64, 3 * n * k).reshape(-1, 3), d_2.download(np.float64, 3 * n * k).reshape(-1, 3)


def dbg_plan_batch(world: "World", can_pass_gate, lo, hi, ns: int, k: int, segs, seqs=(1,), fill: int = 0) -> dict:
    """epp_dbg_plan_batch: one batch through the batched planner's device stages
    (plan_batch_layout / plan_batch_launch), no solver and no fallback.  segs: per problem a
    dict with the caller-filled fields of PlanSeg (seed, s, g, bound, gbound, glo, ghi, h,
    cap).  The batch runs once per entry of seqs on one workspace; fill bit 0: the workspace
    and the pinned block hold 0xFF bytes before the first run, bit 1: the emitted part of
    the pinned block is overwritten with 0xFF between runs.  Returns the last run's emitted
    block: hdr (u64, 3 + 6 S), slots (u32), rows (u16, rows x k), need (doubles, slots x 3),
    row_off / need_off / need_cap per problem, done (the completion slots), nodes (per
    problem its node list from the device) and the layout's sizes."""
    S = len(segs)
    lo = np.ascontiguousarray(lo, np.float64)
    hi = np.ascontiguousarray(hi, np.float64)
    seeds = np.ascontiguousarray([int(q["seed"]) & 0xFFFFFFFFFFFFFFFF for q in segs], np.uint64)
    ends = np.ascontiguousarray([np.concatenate([q["s"], q["g"]]) for q in segs], np.float64)
    bounds = np.ascontiguousarray([[q["bound"], q["gbound"]] for q in segs], np.float64)
    gbox = np.ascontiguousarray([np.concatenate([q["glo"], q["ghi"]]) for q in segs], np.float64)
    h = np.ascontiguousarray([q["h"] for q in segs], np.float64)
    cap = np.ascontiguousarray([q["cap"] for q in segs], np.int32)
    seqs = np.ascontiguousarray(seqs, np.uint32)
    slots_cap = int(np.maximum(cap, 0).sum()) + 4
    need_slots = S * (ns + 4)
    hdr = np.zeros(3 + 6 * S, np.uint64)
    slots = np.zeros(slots_cap, np.uint32)
    rows = np.zeros((slots_cap, k), np.uint16)
    need = np.zeros((need_slots, 3))
    row_off, need_off = np.zeros(S, np.int64), np.zeros(S, np.int64)
    need_cap = np.zeros(S, np.int32)
    done = np.zeros(1024, np.uint32)
    nodes = np.zeros((S, ns + 2, 3))
    meta = np.zeros(6, np.int64)
    check(lib().epp_dbg_plan_batch(world.handle, 1 if can_pass_gate else 0, _ptr(lo), _ptr(hi), int(ns), int(k), S,
                                   _ptr(seeds), _ptr(ends), _ptr(bounds), _ptr(gbox), _ptr(h), _ptr(cap),
                                   _ptr(seqs), len(seqs), int(fill), _ptr(hdr), _ptr(slots), _ptr(rows), slots_cap,
                                   _ptr(need), need_slots, _ptr(row_off), _ptr(need_off), _ptr(need_cap),
                                   _ptr(done), len(done), _ptr(nodes), _ptr(meta)))
    n_nodes = hdr[3 + 3 * S:3 + 4 * S].astype(np.int64)
    return dict(hdr=hdr, slots=slots, rows=rows, need=need, row_off=row_off, need_off=need_off, need_cap=need_cap,
                done=done[:int(meta[2])].copy(), seq=int(seqs[-1]),
                nodes=[nodes[p, :max(0, min(int(n_nodes[p]), ns + 2))].copy() for p in range(S)],
                cap_total=int(meta[0]), need_total=int(meta[1]), ns_log=int(meta[3]), dev_bytes=int(meta[4]),
                host_bytes=int(meta[5]))


def dbg_reverse_csr(nbr: np.ndarray):
    """epp_dbg_reverse_csr: the reverse edges of the masked k-NN table nbr (n x k, -1: none) as
    a CSR built on the device: (roff (n + 1), radj (roff[n] sources, every node's ascending),
    radj16 -- the same as u16 -- or None for n > 65535)."""
    nbr = np.ascontiguousarray(nbr, np.int32)
    n, k = nbr.shape
    d_n = DeviceBuffer.from_array(nbr)
    roff = np.zeros(n + 1, np.int32)
    radj = np.zeros(n * k, np.int32)
    radj16 = np.zeros(n * k, np.uint16) if n <= 65535 else None
    check(lib().epp_dbg_reverse_csr(d_n.ptr, n, k, _ptr(roff), _ptr(radj), _ptr(radj16) if radj16 is not None else None))
    ne = int(roff[n])
    return roff, radj[:ne].copy(), (radj16[:ne].copy() if radj16 is not None else None)


def _dbg_dev(dev: dict, name: str, a, upload: bool):
    """The device buffer of argument `name`: None for None (a NULL pointer), a DeviceBuffer as
    it is, else dev[name], created and filled from the array a on first use and refilled when
    upload is set (else it keeps what it holds)."""
    if a is None or isinstance(a, DeviceBuffer):
        return a
    b = dev.get(name)
    if b is None or b.nbytes < a.nbytes:
        b = dev[name] = DeviceBuffer.from_array(a)
    elif upload:
        b.upload(a)
    return b


def _dbg_back(b, a):
    """The whole of buffer b as an array shaped and typed like a (None for None)."""
    return None if b is None else b.download(a.dtype, a.size).reshape(a.shape)


def dbg_knn_motions_masked(world: "World", nodes, nbr: np.ndarray, can_pass_gate, target: int, valid, out16, count,
                           dev: dict | None = None, upload: bool = True) -> dict:
    """epp_dbg_knn_motions_masked (epp::check_knn_motions_masked): the table nbr (n x k int32)
    over nodes (n x 3, or a DeviceBuffer) with the caller's prefill of every output -- valid
    (n k u8), out16 (n k u16, None: NULL), count (2 i64, None: NULL).  Everything is uploaded,
    the entry runs and every buffer is downloaded whole: dict(rc = the status, nbr = the
    rewritten table, valid, out16, count).  dev: a dict that keeps the device buffers between
    calls; upload=False then runs on what they hold."""
    dev = {} if dev is None else dev
    nbr = np.ascontiguousarray(nbr, np.int32)
    n, k = nbr.shape
    host = dict(nodes=nodes if isinstance(nodes, DeviceBuffer) else np.ascontiguousarray(nodes, np.float64),
                nbr=nbr, valid=None if valid is None else np.ascontiguousarray(valid, np.uint8),
                out16=None if out16 is None else np.ascontiguousarray(out16, np.uint16),
                count=None if count is None else np.ascontiguousarray(count, np.int64))
    d = {name: _dbg_dev(dev, name, a, upload) for name, a in host.items()}
    p = {name: None if b is None else b.ptr for name, b in d.items()}
    rc = lib().epp_dbg_knn_motions_masked(world.handle, p["nodes"], p["nbr"], n, k, 1 if can_pass_gate else 0,
                                          p["valid"], p["out16"], int(target), p["count"], None)
    sync()
    return dict(rc=rc, **{name: _dbg_back(d[name], host[name]) for name in ("nbr", "valid", "out16", "count")})


def dbg_knn_motions_rows_supported(world: "World") -> bool:
    """epp_dbg_knn_motions_rows_supported (epp::knn_motions_rows_supported)."""
    return bool(lib().epp_dbg_knn_motions_rows_supported(world.handle))


def dbg_knn_motions_rows(world: "World", nodes, rows32: np.ndarray, ids32, rows_n: int, can_pass_gate, target: int,
                         valid, out16, count, mark, pkept, pgoal, ns_log: int, nprob: int,
                         dev: dict | None = None, upload: bool = True) -> dict:
    """epp_dbg_knn_motions_rows (epp::check_knn_motions_rows, the marks as plan_batch_launch
    builds them): the packed rows rows32 (cap x k int32, row r = node ids32[r], the first
    rows_n of them live) over nodes (a DeviceBuffer, or an array), with the caller's prefill of
    every output -- valid (cap k u8), out16 (cap k u16), count (2 i64), mark (u8 per node id),
    pkept / pgoal (u64 per problem, and past nprob as far as the caller likes); None: NULL.
    Everything is uploaded, the entry runs and every buffer is downloaded whole:
    dict(rc, rows32, ids32, rows_n, valid, out16, count, mark, pkept, pgoal).  dev / upload: as
    dbg_knn_motions_masked."""
    dev = {} if dev is None else dev
    rows32 = np.ascontiguousarray(rows32, np.int32)
    cap, k = rows32.shape

    def arr(a, dtype):
        return None if a is None else np.ascontiguousarray(a, dtype)

    host = dict(nodes=nodes if isinstance(nodes, DeviceBuffer) else np.ascontiguousarray(nodes, np.float64),
                rows32=rows32, ids32=arr(ids32, np.int32), rows_n=np.array([rows_n], np.int64),
                valid=arr(valid, np.uint8), out16=arr(out16, np.uint16), count=arr(count, np.int64),
                mark=arr(mark, np.uint8), pkept=arr(pkept, np.uint64), pgoal=arr(pgoal, np.uint64))
    d = {name: _dbg_dev(dev, name, a, upload) for name, a in host.items()}
    p = {name: None if b is None else b.ptr for name, b in d.items()}
    rc = lib().epp_dbg_knn_motions_rows(world.handle, p["nodes"], p["rows32"], p["ids32"], p["rows_n"], cap, k,
                                        1 if can_pass_gate else 0, p["valid"], p["out16"], int(target), p["count"],
                                        p["mark"], p["pkept"], p["pgoal"], int(ns_log), int(nprob), None)
    sync()
    return dict(rc=rc, **{name: _dbg_back(d[name], host[name]) for name in host if name != "nodes"})


class Comm:
    """RCCL communicator of the multi-track plan's exchange step (epp_comm_*).

    One process per GPU: Comm(unique_id, n_ranks, rank) on the rank's device, with the
    id from Comm.unique_id() on rank 0 shared out of band."""

    def __init__(self, uid: bytes, n_ranks: int, rank: int, handle=None):
        if handle is not None:
            self.handle = handle
        else:
            assert len(uid) == 128
            buf = (C.c_uint8 * 128).from_buffer_copy(uid)
            h = C.c_void_p()
            check(lib().epp_comm_init(C.cast(buf, C.c_void_p), n_ranks, rank, C.byref(h)))
            self.handle = h.value
        r, n = C.c_int32(), C.c_int32()
        check(lib().epp_comm_rank(self.handle, C.byref(r), C.byref(n)))
        self.rank, self.n_ranks = r.value, n.value

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check(lib().epp_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    @classmethod
    def init_all(cls, devices) -> list["Comm"]:
        devs = np.ascontiguousarray(devices, np.int32)
        hs = (C.c_void_p * len(devs))()
        check(lib().epp_comm_init_all(len(devs), _ptr(devs), C.cast(hs, C.c_void_p)))
        return [cls(b"", 0, 0, handle=h) for h in hs]

    def allgather_waypoints(self, wp: np.ndarray | None, cap: int = 4096) -> list[np.ndarray]:
        """Every rank's (W_r, 3) set.  wp=None: this rank failed (count -1); every rank then
        raises EppError(EPP_ERR_PEER) with `.counts` naming the failed ranks (-1)."""
        out = np.zeros((self.n_ranks, cap, 3))
        counts = np.zeros(self.n_ranks, np.int32)
        if wp is None:
            rc = lib().epp_comm_allgather_waypoints(self.handle, None, -1, cap, _ptr(out), _ptr(counts))
        else:
            wp = np.ascontiguousarray(np.asarray(wp, np.float64).reshape(-1, 3))
            rc = lib().epp_comm_allgather_waypoints(self.handle, _ptr(wp) if len(wp) else None, len(wp), cap,
                                                    _ptr(out), _ptr(counts))
        if rc != EPP_OK:
            err = EppError(rc, lib().epp_last_error().decode())
            err.counts = counts.copy()
            raise err
        return [out[r, :counts[r]].copy() for r in range(self.n_ranks)]

    def allreduce(self, x, op: int = EPP_REDUCE_SUM) -> np.ndarray:
        """x (doubles) reduced over the ranks (epp_comm_allreduce_f64)."""
        a = np.ascontiguousarray(np.array(x, np.float64).reshape(-1))
        check(lib().epp_comm_allreduce_f64(self.handle, _ptr(a), len(a), op))
        return a

    def barrier(self) -> None:
        check(lib().epp_comm_barrier(self.handle))

    def set_timeout(self, seconds: float) -> None:
        """Deadline of every later collective (epp_comm_set_timeout)."""
        check(lib().epp_comm_set_timeout(self.handle, float(seconds)))

    def abort(self) -> None:
        """Request an abort (epp_comm_abort; any thread): the collective in flight, or the
        next one, aborts the communicator and fails."""
        check(lib().epp_comm_abort(self.handle))

    def close(self) -> None:
        if self.handle:
            lib().epp_comm_destroy(self.handle)
            self.handle = None
