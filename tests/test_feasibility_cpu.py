"""CPU checks of the feasibility truth (tests/pyref_feasibility.py: the reference's
formulation of Trajectory::computeMaxVelocityAndAcceleration and
scaleSegmentTimesToMeetConstraints, external/poly_traj/src/trajectory.cpp:344-429) against
hand-made polynomials with known answers and on oracle fits, and the register check of the
k_traj_* kernels (code-object metadata only, no GPU).
"""
import os

import numpy as np
import pytest

import oracle as O
import pyref_feasibility as F
from eppamd import capi, synth
from test_kernel_resources import LLVM, _kernel_metadata


def _seg(x=(), y=(), z=()):
    c = np.zeros((1, 3, 10))
    for d, v in enumerate((x, y, z)):
        c[0, d, :len(v)] = v
    return c


def test_constant_velocity():
    C = _seg(x=(1.0, 0.3), y=(0.0, -0.4), z=(2.0, 1.2))
    pk = F.traj_peaks([2.5], C)
    assert pk[0] == pytest.approx(np.sqrt(0.3 ** 2 + 0.4 ** 2 + 1.2 ** 2), rel=1e-15)
    assert pk[1] == 0.0                 # flat: the earliest time
    assert pk[2] == 0.0 and pk[3] == 0.0


def test_cubic_known_peaks():
    # x(t) = t^2 - t^3 / 3 on [0, 2]: v = 1 - (t - 1)^2, |a| = |2 - 2 t|
    pk = F.traj_peaks([2.0], _seg(x=(0.0, 0.0, 1.0, -1.0 / 3.0)))
    assert pk[0] == pytest.approx(1.0, rel=1e-14) and pk[1] == pytest.approx(1.0, abs=1e-7)
    assert pk[2] == pytest.approx(2.0, rel=1e-14) and pk[3] == 0.0   # 2 at both ends: the earlier


def test_rest_to_rest_peak_at_half_time():
    wp = np.array([[0.0, 0.0, 1.0], [3.0, -2.0, 1.5]])
    T, Cf = O.minsnap_track(wp, 1.0, 2.0)
    pk = F.traj_peaks(T, Cf)
    assert pk[1] == pytest.approx(T[0] / 2, rel=1e-6)
    # the symmetric 9th-order rest-to-rest profile peaks at 315/128 of the mean speed
    assert pk[0] == pytest.approx(315.0 / 128.0 * np.linalg.norm(wp[1] - wp[0]) / T[0], rel=1e-8)
    # and a dense sampling finds nothing higher
    ts = np.linspace(0, T[0], 4001)
    assert max(F.magnitude(Cf[0], t, 1) for t in ts) <= pk[0] * (1 + 1e-12)
    assert max(F.magnitude(Cf[0], t, 2) for t in ts) <= pk[2] * (1 + 1e-12)


def test_second_segment_time_is_from_track_start():
    # the cubic above after a slow constant-velocity segment: its peaks move by that segment's time
    C = np.concatenate([_seg(x=(0.0, 0.1)), _seg(x=(0.0, 0.0, 1.0, -1.0 / 3.0))])
    pk = F.traj_peaks([0.75, 2.0], C)
    assert pk[0] == pytest.approx(1.0, rel=1e-14) and pk[1] == pytest.approx(1.75, abs=1e-7)
    assert pk[2] == pytest.approx(2.0, rel=1e-14) and pk[3] == 0.75


def test_scaling_loop_on_oracle_fits():
    rs = np.random.RandomState(5)
    scaled = 0
    for k in range(50):
        n_seg = (1, 2, 5, 12)[k % 4]
        wp = synth.random_track_waypoints(20000 + k, n_seg)
        T, Cf = O.minsnap_track(wp, 1.0, 2.0)
        v_max, a_max = ((1.0, 2.0), (3.0, 0.6))[k % 2]
        T2, C2, s, within, rounds = F.scale_to_limits(T, Cf, v_max, a_max)
        assert within and rounds <= 2, (k, rounds)
        pk = F.traj_peaks(T2, C2)
        assert pk[0] <= v_max * (1 + 1e-3) and pk[2] <= a_max * (1 + 1e-3)
        if rounds == 0:
            assert s == 1.0 and np.array_equal(T2, T) and np.array_equal(C2, Cf)
            continue
        scaled += 1
        assert s > 1.0
        np.testing.assert_allclose(T2, T * s, rtol=1e-12)
        for tau in rs.uniform(0, T.sum(), 5):   # the same path, s times slower
            assert np.abs(F.position(T2, C2, s * tau) - F.position(T, Cf, tau)).max() < 1e-9
    assert scaled >= 25


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="ROCm LLVM tools absent")
def test_feasibility_kernels_do_not_spill():
    meta = {k: v for k, v in _kernel_metadata(capi.LIB_PATH).items() if "k_traj_" in k}
    assert any("k_traj_peaks" in k for k in meta) and any("k_traj_scale" in k for k in meta), sorted(meta)
    for name, v in meta.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (name, v)
