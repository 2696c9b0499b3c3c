"""The definition of gate passage (include/epp.h: epp_gates_crossed, epp_traj_gate_pass_batch)
restated in numpy: the same IEEE fp64 operations in the same association, nothing fused, and
the ordered resolution as a plain loop over sampled rows.

A frame table is (G, 5): [cx, cy, cz, cos(yaw), sin(yaw)].
"""
import numpy as np


def cross(frames, half_edge, s1, s2):
    """Every edge s1[i] -> s2[i] against every gate: a dict of (n, G) arrays: crossed, u (the
    plane parameter, meaningful where crossed), mx, mz (the midpoint offsets), g1y, g2y."""
    f = np.asarray(frames, np.float64).reshape(-1, 5)
    s1 = np.asarray(s1, np.float64).reshape(-1, 3)
    s2 = np.asarray(s2, np.float64).reshape(-1, 3)
    c, s = f[None, :, 3], f[None, :, 4]
    ax, ay, az = (s1[:, None, k] - f[None, :, k] for k in range(3))
    bx, by, bz = (s2[:, None, k] - f[None, :, k] for k in range(3))
    g1x, g1y = c * ax - s * ay, s * ax + c * ay
    g2x, g2y = c * bx - s * by, s * bx + c * by
    mx, mz = (g1x + g2x) / 2, (az + bz) / 2
    with np.errstate(invalid="ignore", divide="ignore"):
        crossed = (g1y < 0) & (g2y > 0) & (np.abs(mx) <= half_edge) & (np.abs(mz) <= half_edge)
        u = g1y / (g1y - g2y)
    return {"crossed": crossed, "u": u, "mx": mx, "mz": mz, "g1y": g1y, "g2y": g2y}


def masks(crossed):
    """(n, G <= 64) booleans -> uint64[n], bit g = gate g."""
    crossed = np.asarray(crossed, bool)
    m = np.zeros(len(crossed), np.uint64)
    for g in range(crossed.shape[1]):
        m |= crossed[:, g].astype(np.uint64) << np.uint64(g)
    return m


def ordered(crossed):
    """The ordered passage over the chords of one track: crossed is (n_chords, G).  c_-1 = 0;
    c_g = the smallest j >= c_g-1 whose chord crosses gate g; the first gate without one and
    every later gate stay -1.  Returns int64[G]."""
    n, G = crossed.shape
    chord = np.full(G, -1, np.int64)
    j = 0
    for g in range(G):
        while j < n and not crossed[j, g]:
            j += 1
        if j == n:
            break
        chord[g] = j
    return chord


def passes(frames, half_edge, rows, crossed=None):
    """(chord[G], time[G], offset[G, 2], n_passed) of one track from its sampled rows (R, 10:
    positions in columns 0 / 3 / 6, time in column 9).  crossed: the (R - 1, G) predicate of its
    chords if it was computed elsewhere (the device's masks), else the restatement's."""
    G = len(frames)
    chord, time, off = np.full(G, -1, np.int64), np.full(G, -1.0), np.full((G, 2), np.nan)
    if len(rows) < 2 or G == 0:
        return chord, time, off, 0
    xyz = rows[:, [0, 3, 6]]
    r = cross(frames, half_edge, xyz[:-1], xyz[1:])
    chord = ordered(r["crossed"] if crossed is None else crossed)
    for g in range(G):
        j = chord[g]
        if j < 0:
            break
        tj, tj1 = rows[j, 9], rows[j + 1, 9]
        time[g] = tj + r["u"][j, g] * (tj1 - tj)
        off[g] = r["mx"][j, g], r["mz"][j, g]
    return chord, time, off, int((chord >= 0).sum())
