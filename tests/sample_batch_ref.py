"""The exact reference of the row sampler (include/epp.h: epp_sample_count, epp_sample_batch),
plain Python and numpy.

A row of a track is [x, vx, ax, y, vy, ay, z, vz, az, t].  Which rows there are -- segment,
time in the segment `tin`, time `tac` -- is the recurrence of csrc/traj_sample.h as
clearance_ref.recurrence restates it (held bit for bit against the device and against
tests/traj_rows_host.cpp elsewhere).

Value columns.  The truth of derivative k in {0, 1, 2} of the polynomial c at tin is

    p = sum_j B[k][j] c_j tin^(j-k),        B[k][j] = j! / (j-k)!

evaluated here in exact integer arithmetic (doubles are integers over powers of two, so the
sum has a common power-of-two denominator and no rounding happens anywhere).  A sampled value
is held to

    |got - p| <= 32 * 2^-53 * S,            S = sum_j B[k][j] |c_j| |tin|^(j-k).

The number is derived, not measured: the device's evaluation (traj_sample.h poly_eval) rounds
each product B[k][j] c_j once (10 roundings) and does at most 9 fused Horner steps, one
rounding each, so the standard running error bound of Horner's rule is gamma_10 ~ 10 u times
S (u = 2^-53); an unfused Horner (the oracle's) rounds twice a step, gamma_20 ~ 20 u.  32 u
covers both and leaves the fused evaluation a factor of three.  What it is meant to reject --
a wrong k, a wrong segment, the neighbouring row's tin, a dropped coefficient -- is off by
about the size of the terms, many orders above it (test_sample_batch_cpu.py applies each).

Position columns additionally equal clearance_ref.horner (the device's fused Horner, the rule
the clearance tests use) bit for bit.  The time column is tac + t0[k], one double addition.
"""
from fractions import Fraction

import numpy as np

import clearance_ref as CR

N = 10
BOUND = Fraction(32, 2 ** 53)  # the bound factor 32 * 2^-53
VALUE_COLS = [[3 * d + k for k in range(3)] for d in range(3)]  # column of (axis d, derivative k)


def falling(j, k):
    """j! / (j-k)!: the coefficient of t^(j-k) in the k-th derivative of t^j."""
    f = 1
    for i in range(k):
        f *= j - i
    return f


def _ratio(x):
    """(n, e) with x = n / 2^e exactly."""
    n, d = float(x).as_integer_ratio()
    return n, d.bit_length() - 1


def exact(c, tin, k, skip=()):
    """(p, S) of the polynomial c (10 doubles, increasing powers) at tin, as exact Fractions:
    the k-th derivative and the sum of its terms' magnitudes.  skip: indices j left out (the
    "dropped coefficient" mutation)."""
    tn, te = _ratio(tin)
    terms = []
    for j in range(k, N):
        if j in skip:
            continue
        cn, ce = _ratio(c[j])
        if cn:
            m = j - k
            terms.append((falling(j, k) * cn * tn ** m, ce + te * m))
    if not terms:
        return Fraction(0), Fraction(0)
    E = max(e for _, e in terms)
    p = sum(n << (E - e) for n, e in terms)
    S = sum(abs(n) << (E - e) for n, e in terms)
    return Fraction(p, 1 << E), Fraction(S, 1 << E)


def within(got, p, S, extra=0):
    """|got - p| <= 32 * 2^-53 * S + extra, decided exactly; a non-finite got is outside."""
    if not np.isfinite(got):
        return False
    return abs(Fraction(float(got)) - p) <= BOUND * S + Fraction(extra)


def ratio(got, p, S):
    """|got - p| / (32 * 2^-53 * S) as a float for reports (0 / 0 = 0, x / 0 = inf)."""
    if not np.isfinite(got):
        return np.inf
    err = abs(Fraction(float(got)) - p)
    if S == 0:
        return 0.0 if err == 0 else np.inf
    return float(err / (BOUND * S))


class Truth:
    """The rows of one track: seg / tin / tac from the recurrence; p[r][d][k], S[r][d][k] the
    exact values and term sums; pos (R x 3) the positions by clearance_ref.horner."""

    def __init__(self, T, Cf, dt):
        self.T = np.asarray(T, np.float64).ravel()
        self.C = np.asarray(Cf, np.float64).reshape(-1, 3, N)
        self.seg, self.tin, self.tac = CR.recurrence(self.T, dt)
        R = len(self.seg)
        self.p = [[[None] * 3 for _ in range(3)] for _ in range(R)]
        self.S = [[[None] * 3 for _ in range(3)] for _ in range(R)]
        self.pos = np.empty((R, 3))
        for r in range(R):
            for d in range(3):
                c = self.C[self.seg[r], d]
                for k in range(3):
                    self.p[r][d][k], self.S[r][d][k] = exact(c, self.tin[r], k)
                self.pos[r, d] = CR.horner(c, float(self.tin[r]))

    def __len__(self):
        return len(self.seg)

    def time(self, t0=0.0):
        """The time column: tac + t0, one addition."""
        return self.tac + np.float64(t0)

    def ratios(self, rows, extra=0):
        """(ok (R x 3 x 3) by `within`, |got - p| / bound (R x 3 x 3) floats) of the value
        columns of rows (R x >= 9) against this truth."""
        R = len(self)
        assert rows.shape[0] == R, (rows.shape, R)
        ok = np.zeros((R, 3, 3), bool)
        q = np.zeros((R, 3, 3))
        for r in range(R):
            for d in range(3):
                for k in range(3):
                    g = rows[r, VALUE_COLS[d][k]]
                    ok[r, d, k] = within(g, self.p[r][d][k], self.S[r][d][k], extra)
                    q[r, d, k] = ratio(g, self.p[r][d][k], self.S[r][d][k])
        return ok, q


def assert_rows(rows, truth, t0=0.0, what="", extra=0, positions=True):
    """All ten columns of one track's rows against its Truth.  Returns the worst
    |got - p| / bound per derivative order (3 floats)."""
    assert rows.shape == (len(truth), 10), (what, rows.shape, len(truth))
    if len(truth) == 0:
        return np.zeros(3)
    exp_t = truth.time(t0)
    assert rows[:, 9].tobytes() == exp_t.tobytes(), (what, "time column", rows[:, 9], exp_t)
    ok, q = truth.ratios(rows, extra)
    worst = q.max(axis=(0, 1))
    if not ok.all():
        r, d, k = (int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError((what, "row", r, "axis", d, "derivative", k, "segment", int(truth.seg[r]), "tin",
                              float(truth.tin[r]), "got", float(rows[r, VALUE_COLS[d][k]]), "truth",
                              float(truth.p[r][d][k]), "error / bound", q[r, d, k]))
    if positions:
        got = np.ascontiguousarray(rows[:, [0, 3, 6]])
        assert got.tobytes() == truth.pos.tobytes(), (what, "positions differ from the fused Horner",
                                                      np.argwhere(got != truth.pos)[:4].tolist())
    return worst


# ---- the four mistakes the bound is meant to reject ----------------------------------------
MUTATIONS = ("order", "segment", "tin", "drop9")


def mutated(truth, r, d, k, kind):
    """The exact value a sampler with one mistake gives in (row r, axis d, derivative k), or
    None where the mistake has nothing to act on (no next segment, no following row)."""
    seg, tin = int(truth.seg[r]), truth.tin[r]
    if kind == "order":  # derivative k + 1
        return exact(truth.C[seg, d], tin, k + 1)[0]
    if kind == "segment":  # the next segment's coefficients
        return exact(truth.C[seg + 1, d], tin, k)[0] if seg + 1 < len(truth.C) else None
    if kind == "tin":  # tin of the following row
        return exact(truth.C[seg, d], truth.tin[r + 1], k)[0] if r + 1 < len(truth) else None
    assert kind == "drop9"  # c_9 dropped
    return exact(truth.C[seg, d], tin, k, skip=(N - 1,))[0]


def mutation_rejected(truth, kind):
    """True if the mistake `kind` leaves the bound in at least one (row, axis, derivative)."""
    for r in range(len(truth)):
        for d in range(3):
            for k in range(3):
                m = mutated(truth, r, d, k, kind)
                if m is not None and abs(m - truth.p[r][d][k]) > BOUND * truth.S[r][d][k]:
                    return True
    return False
