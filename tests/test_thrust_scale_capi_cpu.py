"""CPU: the argument checks of epp_traj_thrust_grid_batch, epp_traj_scale_to_thrust_limits and
epp_generate_trajectory_flyable_host.  They precede every device call, so they run without a
GPU wherever the library loads."""
import ctypes as C

import numpy as np
import pytest

from eppamd import capi

G = 9.81
NAN, INF = float("nan"), float("inf")
OK = (G, 0.0, INF, INF, -1.0)  # every limit off


def _limits(**kw):
    names = ("g", "f_min", "f_max", "rate_max", "cos_tilt_min")
    return tuple(kw.get(n, v) for n, v in zip(names, OK))


BAD_LIMITS = {
    "g 0": _limits(g=0.0), "g < 0": _limits(g=-G), "g NaN": _limits(g=NAN), "g inf": _limits(g=INF),
    "f_min < 0": _limits(f_min=-1.0), "f_min = g": _limits(f_min=G), "f_min NaN": _limits(f_min=NAN),
    "f_max = g": _limits(f_max=G), "f_max NaN": _limits(f_max=NAN), "rate_max 0": _limits(rate_max=0.0),
    "rate_max NaN": _limits(rate_max=NAN), "cos_tilt_min 1": _limits(cos_tilt_min=1.0),
    "cos_tilt_min NaN": _limits(cos_tilt_min=NAN),
}


def test_scale_to_thrust_limits_argument_checks():
    L = capi.lib()
    p = np.zeros(64).ctypes.data  # a stand-in for device pointers: every case is rejected before anything is read
    bad = capi.EPP_ERR_INVALID_ARGUMENT
    for name, lim in BAD_LIMITS.items():
        assert L.epp_traj_scale_to_thrust_limits(p, p, p, 1, *lim, p, p, p, None) == bad, name
        assert b"epp_traj_scale_to_thrust_limits" in L.epp_last_error(), name
        assert L.epp_traj_scale_to_thrust_limits(None, None, None, 0, *lim, None, None, None, None) == bad, name
    for name, a in {
        "n_tracks < 0": (p, p, p, -1, *OK, p, p, p), "NULL seg_times": (None, p, p, 1, *OK, p, p, p),
        "NULL coeffs": (p, None, p, 1, *OK, p, p, p), "NULL wp_offsets": (p, p, None, 1, *OK, p, p, p),
        "NULL scale": (p, p, p, 1, *OK, None, p, p), "NULL status": (p, p, p, 1, *OK, p, None, p),
    }.items():
        assert L.epp_traj_scale_to_thrust_limits(*a, None) == bad, name
        assert b"epp_traj_scale_to_thrust_limits" in L.epp_last_error(), name
    # an empty batch is fine, with or without buffers, and launches nothing
    assert L.epp_traj_scale_to_thrust_limits(None, None, None, 0, *OK, None, None, None, None) == capi.EPP_OK
    assert L.epp_traj_scale_to_thrust_limits(None, None, None, 0, G, 4.0, 20.0, 3.0, 0.5, None, None, None,
                                             None) == capi.EPP_OK


def test_thrust_grid_argument_checks():
    L = capi.lib()
    p = np.zeros(64).ctypes.data
    bad = capi.EPP_ERR_INVALID_ARGUMENT
    for name, a in {
        "n_tracks < 0": (p, p, p, -1, p, G, p), "g NaN": (p, p, p, 1, p, NAN, p), "g inf": (p, p, p, 1, None, INF, p),
        "NULL seg_times": (None, p, p, 1, p, G, p), "NULL coeffs": (p, None, p, 1, p, G, p),
        "NULL wp_offsets": (p, p, None, 1, p, G, p), "NULL out": (p, p, p, 1, None, G, None),
    }.items():
        assert L.epp_traj_thrust_grid_batch(*a, None) == bad, name
        assert b"epp_traj_thrust_grid_batch" in L.epp_last_error(), name
    assert L.epp_traj_thrust_grid_batch(None, None, None, 0, None, G, None, None) == capi.EPP_OK


def test_wrappers_raise():
    with pytest.raises(capi.EppError) as e:
        capi.check(capi.lib().epp_traj_scale_to_thrust_limits(None, None, None, 0, G, 0.0, 5.0, INF, -1.0, None, None,
                                                              None, None))
    assert e.value.code == capi.EPP_ERR_INVALID_ARGUMENT and "f_min < g < f_max" in str(e.value)
    rows, n = C.POINTER(C.c_double)(), C.c_int64(0)
    wp = np.zeros((1, 3))
    rc = capi.lib().epp_generate_trajectory_flyable_host(wp.ctypes.data, 1, 1.0, 2.0, 0.1, 0.0, None, None, 0, *OK,
                                                         C.byref(rows), C.byref(n), None, None)
    assert rc == capi.EPP_ERR_INVALID_ARGUMENT and b"At least two waypoints" in capi.lib().epp_last_error()
    rc = capi.lib().epp_generate_trajectory_flyable_host(wp.ctypes.data, 1, 1.0, 2.0, 0.1, 0.0, None, None, 0, *OK,
                                                         None, C.byref(n), None, None)
    assert rc == capi.EPP_ERR_INVALID_ARGUMENT
