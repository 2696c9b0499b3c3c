"""CPU: the inputs of test_gpu_minsnap_constrained.py are well enough conditioned for the
oracle to judge the device.

The device is compared with oracle.minsnap_solve to the project's 1e-6.  On every input the GPU
tests use, that oracle must be within 1e-7 of the refined truth (constrained_fit_ref: the KKT
system in long double, LU with four rounds of refinement), which leaves nine tenths of the
1e-6 for the device.  This is a condition on the inputs: a case that misses it gets another
seed in constrained_fit_inputs.py, none is left out.
"""
import numpy as np

import constrained_fit_inputs as CI
import constrained_fit_ref as CR
import minsnap_np

ORACLE_TOL = 1e-7


def test_refined_truth_against_plain_restatement():
    """The ref module restates minsnap_np.solve's system: its plain solve agrees with
    minsnap_np.solve to the accuracy of a double-precision LU of that matrix, and the layouts
    (fixed dict, oracle tables) describe the same problem."""
    for c in (CI.batch(5)[0], CI.batch(5)[1], CI.batch(5)[2], CI.shape_batch()[-1]):
        fixed = c.fixed_dict()
        a = minsnap_np.solve(fixed, len(c.wp), c.T, 3)
        b = CR.solve_refined(fixed, len(c.wp), c.T, 3, plain=True)
        t = CR.solve_refined(fixed, len(c.wp), c.T, 3)
        assert np.abs(a - b).max() < 1e-8, c.what
        assert np.abs(t - b).max() < 1e-8, c.what
        m, val = c.oracle_tables()
        assert m[:, 0].all() and m[0].all() and m[-1].all()
        assert np.isfinite(val[m.astype(bool)]).all()


def test_inputs_cover_the_three_kinds():
    for n_seg in CI.SEGMENTS:
        b = CI.batch(n_seg)
        assert len(b) == CI.N_TRACKS
        if n_seg >= 4:  # random subsets: both pinned and free inner waypoints, both derivatives
            inner = np.concatenate([c.mask[1:-1] for c in b[0::3]])
            assert set(inner.tolist()) == {0, 1, 2, 3}
        assert all((c.mask[1:-1] == 1).all() for c in b[1::3])
        assert all(np.abs(c.values[-1, :2]).min() > 0 and np.abs(c.values[0, 2:]).min() > 0 for c in b[2::3])
        # unused inner slots hold NaN: the fit must never read them
        for c in b:
            assert np.isnan(c.values[~c.used()]).all()
    assert sorted({len(c.T) for c in CI.ragged_batch()})[0] == 1 and max(len(c.T) for c in CI.ragged_batch()) == 30


def test_oracle_within_a_tenth_of_the_tolerance_on_every_input():
    worst, where = 0.0, None
    for c in CI.all_cases():
        truth = CR.solve_refined(c.fixed_dict(), len(c.wp), c.T, 3)
        err = np.abs(c.oracle_coeffs() - truth).max()
        if err > worst:
            worst, where = err, c.what
        assert err < ORACLE_TOL, (c.what, err)
    print(f"oracle vs refined truth: worst {worst:.3e} ({where})")
