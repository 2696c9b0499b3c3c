"""CPU restatement of the time scaling to thrust, body-rate and tilt limits (include/epp.h:
epp_traj_thrust_grid_batch, epp_traj_scale_to_thrust_limits; csrc/thrust_scale.h) in numpy
float64, one rounded operation per step (the device code calls no fma here).

Grid points: segment m of time T_m gives tau_i = T_m * (i * (1 / 64)), i = 0..63, and tau = T_m;
a = p''(tau), j = p'''(tau) by Horner over the derivative's coefficients (r = r * t + f_j * c_j,
a multiply and an add); a point's time is the in-order sum of the earlier segment times plus tau.
At scale s: s2 = s * s, s3 = s2 * s, a / s2, j / s3, then thrust_rates_ref.samples.  A point
violates when thrust < f_min (1), thrust > f_max (2), rate > rate_max (4), cos_tilt <
cos_tilt_min (8); a NaN violates nothing.  The search: feasible at 1 -> (1.0, status 0); hi = 2
doubled while infeasible up to 1024 (infeasible there: status 1, scale 1.0); lo = hi / 2 and 12
rounds of mid = 0.5 * (lo + hi), hi = mid when feasible else lo = mid; the answer is hi.  The
apply: T * s, and c[n] * f with f = f * (1 / s).

VARIANTS: the same with one mistake each, for the mutation tests.
"""
import collections

import numpy as np

import clearance_ref as CR
import thrust_rates_ref as TR

N = 10
POINTS = 64
MAX_DOUBLINGS = 10
BISECT_ROUNDS = 12
MARGIN_ULPS = 4.0
F_MIN, F_MAX, RATE, TILT = 1, 2, 4, 8
IDENTITY = TR.IDENTITY
VARIANTS = (None, "a / s3", "reciprocal", "hi from an infeasible mid", "11 rounds", "tau = T dropped")

Limits = collections.namedtuple("Limits", "g f_min f_max rate_max cos_tilt_min")


def limits_ok(L):
    return bool(0.0 < L.g < np.inf and 0.0 <= L.f_min < L.g < L.f_max and L.rate_max > 0.0 and L.cos_tilt_min < 1.0)


def falling(j, k):
    f = 1.0
    for i in range(k):
        f *= float(j - i)
    return f


def deriv(c, t, k):
    """deriv<K>: c (..., 10), t broadcastable; a multiply and an add per Horner step."""
    c = np.asarray(c, np.float64)
    t = np.asarray(t, np.float64)
    r = falling(N - 1, k) * c[..., N - 1] * np.ones_like(t)
    for j in range(N - 2, k - 1, -1):
        r = r * t + falling(j, k) * c[..., j]
    return r


def track_invalid(T, Cf):
    T = np.asarray(T, np.float64).ravel()
    Cf = np.asarray(Cf, np.float64)
    return bool(len(T) < 1 or not (np.isfinite(T) & (T > 0.0)).all() or not np.isfinite(Cf).all())


class Grid:
    """The grid points of one track: a, j (P, 3), time (P,), in order (65 per segment)."""

    def __init__(self, T, Cf, variant=None):
        T = np.asarray(T, np.float64).ravel()
        Cf = np.asarray(Cf, np.float64).reshape(-1, 3, N)
        acc, jerk, time = [], [], []
        start = np.float64(0.0)
        for m in range(len(T)):
            tau = np.append(T[m] * (np.arange(POINTS) * (1.0 / POINTS)), T[m])
            if variant == "tau = T dropped":
                tau = tau[:-1]
            acc.append(deriv(Cf[m][None, :, :], tau[:, None], 2))
            jerk.append(deriv(Cf[m][None, :, :], tau[:, None], 3))
            time.append(start + tau)
            start = start + T[m]
        self.acc, self.jerk, self.time = np.concatenate(acc), np.concatenate(jerk), np.concatenate(time)

    def at(self, s, g, variant=None):
        """(thrust, rate, cos_tilt) of every point at scale s."""
        s = np.float64(s)
        s2 = s * s
        s3 = s2 * s
        with np.errstate(all="ignore"):
            if variant == "a / s3":
                a, j = self.acc / s3, self.jerk / s3
            elif variant == "reciprocal":
                a, j = self.acc * (1.0 / s2), self.jerk * (1.0 / s3)
            else:
                a, j = self.acc / s2, self.jerk / s3
        return TR.samples(a, j, g, None)[:3]


def violation(q, L):
    """The OR of the points' violation bits; q = (thrust, rate, cos_tilt)."""
    f, w, c = q
    with np.errstate(invalid="ignore"):
        return ((F_MIN if (f < L.f_min).any() else 0) | (F_MAX if (f > L.f_max).any() else 0) |
                (RATE if (w > L.rate_max).any() else 0) | (TILT if (c < L.cos_tilt_min).any() else 0))


def marginal(q, L):
    """True when some point's quantity lies within MARGIN_ULPS ulp of a finite limit it is
    compared with, so a rounding difference of a root could turn the decision."""
    f, w, c = q
    close = False
    for v, lim in ((f, L.f_min), (f, L.f_max), (w, L.rate_max), (c, L.cos_tilt_min)):
        if np.isfinite(lim):
            v = v[np.isfinite(v)]
            close = close or bool((np.abs(v - lim) <= MARGIN_ULPS * np.spacing(abs(lim))).any())
    return close


def search_steps(variant=None):
    """The search as a generator: yields the scale to evaluate next, is sent the violation bits
    there, returns (scale, status, violated at 1)."""
    first = yield 1.0
    if not first:
        return 1.0, 0, 0
    hi, d = 2.0, 1
    while True:
        bad = yield hi
        if not bad:
            break
        if d == MAX_DOUBLINGS:
            return 1.0, 1, first
        hi, d = hi * 2.0, d + 1
    lo = hi * 0.5
    for _ in range(BISECT_ROUNDS - (1 if variant == "11 rounds" else 0)):
        mid = 0.5 * (lo + hi)
        bad = yield mid
        if variant == "hi from an infeasible mid":
            bad = not bad
        if bad:
            lo = mid
        else:
            hi = mid
    return hi, 0, first


def search(violated_at, variant=None):
    """(scale, status, violated at 1, the scales visited)."""
    gen, seen = search_steps(variant), []
    try:
        s = next(gen)
        while True:
            seen.append(s)
            s = gen.send(violated_at(s))
    except StopIteration as e:
        return (*e.value, seen)


def apply(T, Cf, s):
    """One round of k_traj_scale: (T * s, coefficients through scalePolynomialInTime(1 / s))."""
    T = np.asarray(T, np.float64).ravel()
    Cn = np.array(Cf, np.float64).reshape(-1, 3, N)
    inv = 1.0 / np.float64(s)
    f = np.float64(1.0)
    for n in range(N):
        Cn[:, :, n] = Cn[:, :, n] * f
        f = f * inv
    return T * np.float64(s), Cn


Result = collections.namedtuple("Result", "scale status violated T C seen marginal")


def scale_track(T, Cf, L, variant=None):
    """epp_traj_scale_to_thrust_limits of one track."""
    T = np.asarray(T, np.float64).ravel()
    Cf = np.asarray(Cf, np.float64).reshape(-1, 3, N)
    if track_invalid(T, Cf):
        return Result(1.0, -1, 0, T, Cf, [], False)
    grid = Grid(T, Cf, variant)
    close = []

    def violated_at(s):
        q = grid.at(s, L.g, variant)
        close.append(marginal(q, L))
        return violation(q, L)

    scale, status, first, seen = search(violated_at, variant)
    if status == 0 and scale != 1.0:
        T, Cf = apply(T, Cf, scale)
    return Result(scale, status, first, T, Cf, seen, any(close))


def scale_tracks(Ts, Cs, L, variant=None):
    return [scale_track(T, Cf, L, variant) for T, Cf in zip(Ts, Cs)]


def grid_extremes(T, Cf, s, g, variant=None):
    """epp_traj_thrust_grid_batch of one track: (out[8], the point indices [4], Grid values)."""
    if track_invalid(T, Cf):
        return IDENTITY.copy(), np.full(4, -1, np.int64), None
    grid = Grid(T, Cf, variant)
    q = grid.at(s, g, variant)
    out, idx = TR.reduce(q[0], q[1], q[2], grid.time)
    return out, idx, q


# ---- the comparisons of test_gpu_thrust_scale.py ----------------------------------------------
def compare_results(got, exp, skip=None):
    """[(track, what)] where (scale, status, violated, T, C) of the tracks differ at all; got
    and exp: sequences of Result-like tuples (scale, status, violated, T, C, ...).  Tracks in
    `skip` are left out."""
    bad = []
    for k, (a, b) in enumerate(zip(got, exp)):
        if skip is not None and k in skip:
            continue
        if not a[0] == b[0]:
            bad.append((k, "scale"))
        if a[1] != b[1]:
            bad.append((k, "status"))
        if a[2] != b[2]:
            bad.append((k, "violated"))
        if np.asarray(a[3]).tobytes() != np.asarray(b[3]).tobytes():
            bad.append((k, "seg_times"))
        if np.asarray(a[4]).tobytes() != np.asarray(b[4]).tobytes():
            bad.append((k, "coeffs"))
    return bad


def compare_grid(got_out, exp_out, by_time):
    """[(track, column)] where thrust_grid's extremes differ from the restatement's: values
    beyond thrust_rates_ref's ulps or in their NaN / inf positions, and -- for the (track,
    quantity) pairs of by_time, those whose extreme is separated from the runner-up -- the times."""
    bad = []
    for k in range(len(exp_out)):
        for c in range(8):
            if c % 2 == 1:
                if by_time[k][c // 2] and not got_out[k, c] == exp_out[k, c]:
                    bad.append((k, c))
            elif TR._differs(got_out[k, c], exp_out[k, c], TR.OUT_ULPS[c]):
                bad.append((k, c))
    return bad


def extremes_violation(o, L):
    """The violation bits from the grid extremes out[8] of one track: "some point violates" is
    "an extreme lies outside its limit"."""
    return ((F_MIN if o[0] < L.f_min else 0) | (F_MAX if o[2] > L.f_max else 0) |
            (RATE if o[4] > L.rate_max else 0) | (TILT if o[6] < L.cos_tilt_min else 0))


def composition(grid_call, valid, L):
    """The search driven from outside, every track of a batch in step: grid_call(scales (n,))
    -> out (n, 8), one call per step (at most 1 + 10 + 12); valid[k] False: status -1.  Returns
    (scale (n,), status (n,), violated (n,), number of calls)."""
    n = len(valid)
    scale, status, viol = np.ones(n), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    gens = {k: search_steps() for k in range(n) if valid[k]}
    ask = {k: next(g) for k, g in gens.items()}
    calls = 0
    while ask:
        s = np.ones(n)
        for k, v in ask.items():
            s[k] = v
        out = grid_call(s)
        calls += 1
        for k in list(ask):
            try:
                ask[k] = gens[k].send(extremes_violation(out[k], L))
            except StopIteration as e:
                scale[k], status[k], viol[k] = e.value
                del ask[k]
    return scale, status, viol, calls
