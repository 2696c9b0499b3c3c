"""CPU restatement of the thrust / body-rate calls (include/epp.h: epp_sample_derivative_batch,
epp_thrust_rates, epp_traj_thrust_rates_batch) in numpy float64 and plain Python.

Per sample (csrc/thrust_rates.h), every operation one IEEE multiply, add, subtract, divide or
square root in the definition's association:

    Fx = ax;  Fy = ay;  Fz = az + g
    f2 = (Fx*Fx + Fy*Fy) + Fz*Fz;       thrust   = sqrt(f2)
    cx = Fy*jz - Fz*jy;  cy = Fz*jx - Fx*jz;  cz = Fx*jy - Fy*jx
    w2 = (cx*cx + cy*cy) + cz*cz;       rate     = sqrt(w2) / f2
                                        cos_tilt = Fz / thrust

Derivative values by the device's rule (csrc/traj_sample.h poly_eval): one rounded product
B[k][j] * c[j] per term, then fused Horner steps (clearance_ref.fma), bit for bit.  The rows are
clearance_ref.recurrence's.  The reductions keep the earliest row that attains an extreme and
update only on strict < or >, so a NaN never does; (+inf | -inf, row -1, time -1.0) without one.

VARIANTS: the same with one mistake each, for the mutation tests.
"""
import numpy as np

import clearance_ref as CR
from sample_batch_ref import N, falling

IDENTITY = np.array([np.inf, -1.0, -np.inf, -1.0, -np.inf, -1.0, np.inf, -1.0])
VARIANTS = (None, "swapped cross terms", "f in the divisor", "non-strict comparison", "order 2 for the jerk")


def samples(acc, jerk, g, variant=None):
    """(thrust, rate, cos_tilt, f2) per sample."""
    a = np.asarray(acc, np.float64).reshape(-1, 3)
    j = np.asarray(jerk, np.float64).reshape(-1, 3)
    g = np.float64(g)
    with np.errstate(all="ignore"):
        Fx, Fy, Fz = a[:, 0], a[:, 1], a[:, 2] + g
        jx, jy, jz = j[:, 0], j[:, 1], j[:, 2]
        f2 = (Fx * Fx + Fy * Fy) + Fz * Fz
        thrust = np.sqrt(f2)
        cx = Fy * jz - Fz * jy
        cy = Fz * jx - Fx * jz
        cz = Fx * jy - Fy * jx
        if variant == "swapped cross terms":  # (cx with the jerk's components swapped)
            cx = Fy * jy - Fz * jz
        w2 = (cx * cx + cy * cy) + cz * cz
        rate = np.sqrt(w2) / (thrust if variant == "f in the divisor" else f2)
        cos_tilt = Fz / thrust
    return thrust, rate, cos_tilt, f2


def deriv(c, t, k):
    """poly_eval(B, c, t, k): the products rounded once each, fused Horner steps."""
    c = [float(v) for v in c]
    t = float(t)
    if not np.isfinite(t):
        return float("nan")
    j = N - 1
    while j > k and c[j] == 0.0:  # (fma(0, t, p) = p for finite t: the leading zeros change nothing)
        j -= 1
    r = float(falling(j, k)) * c[j]
    for i in range(j - 1, k - 1, -1):
        r = CR.fma(r, t, float(falling(i, k)) * c[i])
    return r


def track_values(T, Cf, dt, order, rec=None):
    """(R, 3) derivative `order` of every row of one track."""
    seg, tin, _ = rec if rec is not None else CR.recurrence(T, dt)
    Cf = np.asarray(Cf, np.float64).reshape(-1, 3, N)
    out = np.empty((len(seg), 3))
    for r in range(len(seg)):
        for d in range(3):
            out[r, d] = deriv(Cf[seg[r], d], tin[r], order)
    return out


def reduce(thrust, rate, cos_tilt, time, variant=None):
    """(out[8], rows[4]) of one track from its rows' values and time column."""
    out, rows = IDENTITY.copy(), np.full(4, -1, np.int64)
    for q, (v, is_min) in enumerate(((thrust, True), (thrust, False), (rate, False), (cos_tilt, True))):
        v = np.asarray(v, np.float64)
        ident = np.inf if is_min else -np.inf
        with np.errstate(invalid="ignore"):
            ok = (v < ident) if is_min else (v > ident)  # (a NaN and the identity itself never update)
        if not ok.any():
            continue
        w = np.where(ok, v, ident)
        best = w.min() if is_min else w.max()
        hits = np.flatnonzero(ok & (v == best))
        r = int(hits[-1] if variant == "non-strict comparison" else hits[0])
        out[2 * q], out[2 * q + 1], rows[q] = best, time[r], r
    return out, rows


class Track:
    """One track's rows by the restatement: time column, a, j, the three quantities."""

    def __init__(self, T, Cf, dt, g, variant=None):
        rec = CR.recurrence(np.asarray(T, np.float64).ravel(), dt)
        self.time = rec[2] + 0.0
        self.acc = track_values(T, Cf, dt, 2, rec)
        self.jerk = self.acc if variant == "order 2 for the jerk" else track_values(T, Cf, dt, 3, rec)
        self.thrust, self.rate, self.cos_tilt, self.f2 = samples(self.acc, self.jerk, g, variant)
        self.out, self.rows = reduce(self.thrust, self.rate, self.cos_tilt, self.time, variant)

    def quantities(self):
        """[(values over the rows, is a minimum)] in the order of out / rows."""
        return [(self.thrust, True), (self.thrust, False), (self.rate, False), (self.cos_tilt, True)]


def tracks(Ts, Cs, dt, g, variant=None):
    """(out (K, 8), rows (K, 4), [Track])."""
    tr = [Track(T, Cf, dt, g, variant) for T, Cf in zip(Ts, Cs)]
    return (np.array([t.out for t in tr]).reshape(len(tr), 8), np.array([t.rows for t in tr]).reshape(len(tr), 4),
            tr)


def separated(values, is_min, row, ulps=4.0):
    """True when the extreme values[row] is more than `ulps` ulp from every other row's value
    (the runner-up), so a rounding difference of a few ulp cannot move the answer to another
    row.  NaN rows never take part.  A track whose rows all hold the same bits answers its
    first row whatever the rounding (the same operations on the same inputs): it counts as
    separated.  row == -1 (nothing ever updated): separated."""
    v = np.asarray(values, np.float64)
    if row < 0:
        return True
    live = ~np.isnan(v)
    assert live[row] and row == np.flatnonzero(live & (v == v[row]))[0]
    if (v[live] == v[row]).all():
        return row == np.flatnonzero(live)[0]
    live[row] = False
    runner = v[live].min() if is_min else v[live].max()
    if np.isinf(v[row]) or np.isinf(runner):
        return bool(runner != v[row])
    gap = (runner - v[row]) if is_min else (v[row] - runner)
    return bool(gap > ulps * np.spacing(abs(v[row])))


# ---- the comparisons of test_gpu_thrust_rates.py ---------------------------------------------
# thrust: one square root, which the device may round differently (1 ulp); rate and cos_tilt:
# that root, or one like it, feeding one correctly rounded division (2 ulp).
ULPS = {"thrust": 1.0, "rate": 2.0, "cos_tilt": 2.0}
OUT_ULPS = (ULPS["thrust"], 0.0, ULPS["thrust"], 0.0, ULPS["rate"], 0.0, ULPS["cos_tilt"], 0.0)


def _differs(got, exp, ulps):
    """Elementwise: NaN / inf positions differ, or finite values differ by more than ulps."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    fin = np.isfinite(exp)
    bad = np.where(fin, ~np.isfinite(got), ~((got == exp) | (np.isnan(got) & np.isnan(exp))))
    with np.errstate(invalid="ignore", over="ignore"):
        bad |= fin & np.isfinite(got) & (CR.ulps(got, exp) > ulps)
    return bad


def compare_samples(got, exp):
    """[(quantity, index)] where the per-sample values (thrust, rate, cos_tilt) differ from the
    restatement's by more than their ulps or in their NaN / inf positions."""
    bad = []
    for name, g, e in zip(("thrust", "rate", "cos_tilt"), got, exp):
        bad += [(name, int(i)) for i in np.flatnonzero(_differs(g, e, ULPS[name]))]
    return bad


def compare_tracks(got_out, got_rows, exp_out, exp_rows, by_row=None):
    """[(track, what)] where the fused call's outputs differ from the restatement's: values
    beyond their ulps, and -- for the tracks of by_row (None: all), those that meet the
    separation condition -- the rows and, exactly, their times."""
    bad = []
    for k in range(len(exp_out)):
        rows_too = by_row is None or by_row[k]
        for c in range(8):
            if c % 2 == 1 and not rows_too:
                continue
            if _differs(got_out[k, c], exp_out[k, c], OUT_ULPS[c]):
                bad.append((k, f"out[{c}]"))
        if rows_too and not np.array_equal(got_rows[k], exp_rows[k]):
            bad.append((k, "rows"))
    return bad
