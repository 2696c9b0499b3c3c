"""CPU: every input set of the thrust-limit scaling tests (thrust_scale_inputs.py) does what
its name says, by the restatement alone (thrust_scale_ref.py), and on the fitted sets no
decision of the restatement's search falls within the margin (4 ulp of a limit) that
test_gpu_thrust_scale.py would leave a track out for."""
import functools

import numpy as np

import oracle as O
import thrust_scale_inputs as si
import thrust_scale_ref as sr


@functools.lru_cache(maxsize=None)
def fitted():
    fT, fC, _ = O.minsnap_batch(list(si.fit_waypoints()), si.V_MAX, si.A_MAX, threads=8)
    sT, sC, _ = O.minsnap_batch(list(si.short_waypoints()), si.V_MAX, si.A_MAX, threads=8)
    return list(fT), list(fC), list(sT), list(sC)


def test_hand_built_tracks_give_their_exact_answers():
    groups = si.hand_groups()
    assert {g.name for g in groups} >= {"f_max", "tilt", "rate", "f_min", "free fall"}
    for g in groups:
        assert sr.limits_ok(g.limits)
        for name, T, C, want, r in zip(g.names, g.Ts, g.Cs, g.wants, sr.scale_tracks(g.Ts, g.Cs, g.limits)):
            what = (g.name, name)
            assert (r.status, r.violated) == (want.status, want.violated), what
            if want.scale is not None:
                assert r.scale == want.scale, what
            if r.scale == 1.0:  # untouched, bit for bit
                assert r.T.tobytes() == np.asarray(T, np.float64).tobytes(), what
                assert r.C.tobytes() == np.asarray(C, np.float64).tobytes(), what
            else:
                Tn, Cn = sr.apply(T, C, r.scale)
                assert r.T.tobytes() == Tn.tobytes() and r.C.tobytes() == Cn.tobytes(), what
                # feasible at the answer, infeasible 2^-12 of the bracket below it
                grid = sr.Grid(T, C)
                assert sr.violation(grid.at(r.scale, g.limits.g), g.limits) == 0, what
                assert sr.violation(grid.at(r.seen[-1] if r.seen[-1] < r.scale else r.scale - 2.0 ** -12,
                                            g.limits.g), g.limits) != 0, what
            if want.t_fmax is not None:
                assert sr.grid_extremes(T, C, 1.0, g.limits.g)[0][3] == want.t_fmax, what


def test_free_fall_and_thrust_axis_down():
    g = {x.name: x for x in si.hand_groups()}
    r = sr.scale_tracks(g["free fall"].Ts, g["free fall"].Cs, si.L_FALL)[0]
    assert si.FREE_FALL_SCALE[0] < r.scale < si.FREE_FALL_SCALE[1] and r.violated == sr.F_MIN
    k = g["f_min"].names.index("thrust axis down")
    grid = sr.Grid(g["f_min"].Ts[k], g["f_min"].Cs[k])
    f1, _, c1 = grid.at(1.0, si.G)
    f2, _, _ = grid.at(1.5, si.G)
    assert (f1 == 19.5).all() and (c1 == -1.0).all() and (f2 == 3.25).all()  # feasible at 1, not at 1.5


def test_peaks_sit_where_they_say():
    g = si.hand_groups()[0]
    seen = set()
    for name, T, C in zip(g.names, g.Ts, g.Cs):
        if not name.startswith("peak on"):
            continue
        out, idx, _ = sr.grid_extremes(T, C, 1.5, si.G)
        assert out[2] == 16.25
        seen.add((len(T), int(idx[1]) // 65, int(idx[1]) % 65))
    assert {p for _, _, p in seen} == {0, 1, 31, 63, 64}
    assert {(n, m) for n, m, _ in seen} == set(si.PEAK_PLACES)


def test_fitted_sets():
    fT, fC, sT, sC = fitted()
    assert [len(t) for t in fT] == [3 + k % 10 for k in range(65)] + [si.FIT_LONG]
    assert len(sT) == 41 and all(len(t) == 2 for t in sT) and si.N_SHORT == 41 * 25
    res = sr.scale_tracks(fT, fC, si.L_FIT)
    scales = np.array([r.scale for r in res])
    print("fitted scales: min %.3f median %.3f max %.3f" % (scales.min(), np.median(scales), scales.max()))
    assert all(r.status == 0 for r in res)
    assert ((scales > 1.0) & (scales < 4.0)).mean() > 0.5  # most need 1 < s < 4
    assert res[-1].scale > 1.0  # the 44-segment set is scaled too
    assert {r.violated & b for r in res for b in (1, 2, 4, 8)} >= {1, 2, 4, 8}  # every limit binds somewhere
    short = sr.scale_tracks(sT, sC, si.L_FIT)
    assert sum(r.scale > 1.0 for r in short) > 20 and all(r.status == 0 for r in short)
    # no search decision within the margin: the GPU comparison leaves none of them out
    assert not any(r.marginal for r in res) and not any(r.marginal for r in short)
