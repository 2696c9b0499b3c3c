"""Worlds far from the origin, and the states, edges and hover tracks that probe them
(test_far_world_inputs_cpu.py, test_gpu_far_worlds.py).

Every spatial index of the collision kernels (the cull grid, the class grid, the motion tiles)
is built in float over double data.  Within a few metres of the origin (float)p resolves 1e-6 m
and the index's arguments are never under load; here the C2 track stands about 1 km and about
100 km away, where (float)p resolves 6e-5 m and 8e-3 m, AABB faces and states share float
images, and the float extent (float)g1 - (float)g0 of the cull grid is off by ulps of |g|, not
of the extent.

Worlds: synth.track_world(42) under configs/config.json plus four unrotated "cap" obstacles at
about (+-7.5, 0) and (0, +-7.5), whose flat inflated faces are the union's g0 / g1 in x and y;
then (dx, dy) added to the x and y of every gate and obstacle (z stays: gate z is forced to 0).
The caps on the negative side stand at -7.45035 and -7.432465: with all four at exactly 7.5 the
union is 15.5 m wide, a whole number of float spacings at every offset used here, g0 and g1
then round the same way and the float extent is exact wherever the world stands.  With these
the extent ends near the middle of a float spacing at 1 km and at 100 km alike.

    "near"   (0, 0)                     the control
    "km"     (+1001.669, -1002.235)     KM_CANDIDATES[2]: the first that reaches the sliver on +x and +y
    "100km"  (-100000.679, +100003.513) HKM_CANDIDATES[2]: likewise

The sliver: states p with g1[k] - w < p[k] < g1[k] whose fine coordinate ((float)p - (float)g0)
* i4 exceeds 4 n (1 + 2^-20), the limit the cull grid used to cut at: strictly inside the cap's
inflated AABB and inside its inflated OBB, so invalid, yet beyond the cut.  The widest ladder
rung found in it (sliver_width(), float32 numpy) and the number of distinct rungs:

    "km"     +x 1.5e-05 m (26 rungs)   +y 1.5e-05 m (26)   (float spacing at 1 km: 6.1e-05 m)
    "100km"  +x 3.9e-03 m (27 rungs)   +y 9.8e-04 m (25)   (float spacing at 100 km: 7.8e-03 m)

Everything is input data and oracle output: built once per process, shared, read-only.
"""
import ctypes as C
import functools

import numpy as np

import oracle as O
from eppamd import capi, config, synth

from conftest import CONFIG
from small_path_inputs import adversarial_points

# the candidate lists the offsets were picked from: the first of each whose ladder reaches the
# sliver on +x and +y (test_far_world_inputs_cpu.py asserts that the chosen ones do)
KM_CANDIDATES = ((1000.587, -1000.369), (1001.677, -1002.741), (1001.669, -1002.235), (1000.562, -1000.792))
HKM_CANDIDATES = ((-100003.832, 100002.133), (-100001.122, 100003.157), (-100000.679, 100003.513),
                  (-100000.393, 100001.684))
OFFSETS = {"near": (0.0, 0.0), "km": KM_CANDIDATES[2], "100km": HKM_CANDIDATES[2]}
WORLDS = tuple(OFFSETS)
FAR = ("km", "100km")
BUILD_ONLY_OFFSETS = (1e6, 1e7)  # index build and cull-grid property only

CAPS = ((7.5, 0.0), (-7.45035, 0.0), (0.0, 7.5), (0.0, -7.432465))
MIN_DISTANCES = (0.2, 0.3)  # both >= the inflate radii: a sliver state is inside the md-inflated cap
N_STATES = 8191   # = 3 mod 4, past the brute-force path's 4096
N_EDGES = 4099    # = 3 mod 4, past the brute-force path's 1024
LADDER_REPS = 3   # states per rung
ULP_RUNGS = (1, 2, 4)
POW_RUNGS = 25    # s * 2^-j, j = 0..24
T_HOVER = 0.2
DT = 0.05


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def setup():
    """(geometry, r_gate, r_obst) of configs/config.json."""
    cfg = config.load(CONFIG)
    return (config.geometry(cfg),) + tuple(config.inflate_radii(cfg))


@functools.lru_cache(maxsize=None)
def poses_at(dx, dy):
    gates, obstacles = synth.track_world(42)
    gates, obstacles = np.array(gates, float), np.array(obstacles, float)
    caps = np.zeros((len(CAPS), 6))
    caps[:, :2] = CAPS
    obstacles = np.vstack([obstacles, caps])
    gates[:, 0] += dx
    gates[:, 1] += dy
    obstacles[:, 0] += dx
    obstacles[:, 1] += dy
    return _frozen(gates, obstacles)


@functools.lru_cache(maxsize=None)
def world_at(dx, dy):
    """(OBBs for capi.World, the oracle's world) of the capped track moved by (dx, dy)."""
    geom, rg, ro = setup()
    gates, obstacles = poses_at(dx, dy)
    obbs = capi.build_obbs(geom, gates, obstacles)
    ref = O.world_build(geom, gates, obstacles, rg, ro)
    assert len(obbs) == len(ref) == 5 * len(gates) + len(obstacles)
    # the caps' flat faces are the union's g0 / g1 in x and y
    n, lo, hi = len(ref), ref["aabb_lo"], ref["aabb_hi"]
    for j, (k, top) in enumerate(((0, True), (0, False), (1, True), (1, False))):
        i = n - len(CAPS) + j
        assert (hi[i, k] == hi[:, k].max() and (hi[:i, k] < hi[i, k]).all()) if top else \
               (lo[i, k] == lo[:, k].min() and (lo[:i, k] > lo[i, k]).all()), (j, k, top)
        assert ref["rot"][i][0] == 1.0 and ref["rot"][i][3] == 0.0
    return _frozen(obbs, ref)


def poses(name):
    return poses_at(*OFFSETS[name])


def world(name):
    return world_at(*OFFSETS[name])


def bounds(name):
    """(g0, g1): the union of the oracle's AABBs."""
    _, ref = world(name)
    return ref["aabb_lo"].min(axis=0), ref["aabb_hi"].max(axis=0)


# ---- the host index build's debug entries ------------------------------------------------------
def cull_grid(obbs):
    """epp_dbg_cull_grid: dict of n (3 ints) and of, i4, lim, fmax (float32[3]), g0, g1 (float64[3])."""
    _, rg, ro = setup()
    f = capi.lib().epp_dbg_cull_grid
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p]
    out = np.zeros(21)
    obbs = np.ascontiguousarray(obbs)
    capi.check(f(obbs.ctypes.data, len(obbs), rg, ro, out.ctypes.data))
    g = {"n": out[0:3].astype(np.int64), "g0": out[15:18].copy(), "g1": out[18:21].copy()}
    for j, key in enumerate(("of", "i4", "lim", "fmax")):
        g[key] = out[3 + 3 * j: 6 + 3 * j].astype(np.float32)
        assert np.array_equal(g[key].astype(np.float64), out[3 + 3 * j: 6 + 3 * j])  # they are floats
    return g


def build_blob(obbs, reps=1):
    """epp_dbg_build_blob: (status, dict of us, blob_bytes, tile_n, tile_words, slab_w, slab_n)."""
    _, rg, ro = setup()
    f = capi.lib().epp_dbg_build_blob
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p]
    out = np.zeros(6)
    obbs = np.ascontiguousarray(obbs)
    st = f(obbs.ctypes.data, len(obbs), rg, ro, reps, out.ctypes.data)
    return st, dict(zip("us blob_bytes tile_n tile_words slab_w slab_n".split(), out.tolist()))


def class_layout(obbs):
    """epp_dbg_class_layout as a dict (staged: the bytes k_states_v5 stages)."""
    _, rg, ro = setup()
    f = capi.lib().epp_dbg_class_layout
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p]
    out = np.zeros(12, np.int64)
    obbs = np.ascontiguousarray(obbs)
    capi.check(f(obbs.ctypes.data, len(obbs), rg, ro, out.ctypes.data))
    return dict(zip("aos lists ids cls8 bitmap blob nlists cells bnx bny bnz staged".split(), out.tolist()))


def fine_coord(p, o, i4):
    """epp_internal.h fine_coord in numpy float32: ((float)p - o) * inv4, each step rounded."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(p, np.float64).astype(np.float32) - np.float32(o)) * np.float32(i4)


def old_limit(n):
    """4 n (1 + 2^-20) in float: where the cull grid used to cut, the bound that was not enough."""
    return np.float32(4 * int(n)) * (np.float32(1.0) + np.float32(2.0 ** -20))


# ---- the sliver ladder -----------------------------------------------------------------------
def _nudged(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def _local_to_world(o, l):
    c, s = o["rot"][0], o["rot"][3]
    return o["center"] + np.array([c * l[0] - s * l[1], s * l[0] + c * l[1], l[2]])


@functools.lru_cache(maxsize=None)
def ladder(name):
    """The sliver ladder.  Per axis k and end of the union (the face g = g1[k] or g0[k], attained
    by OBB i: a cap in x and y, the tallest / lowest OBB in z), per rung d (1, 2, 4 double ulps of
    g; s 2^-j, j = 0..24, s = the float spacing at |g|) LADDER_REPS states with p[k] = g -+ d and
    the other two coordinates uniform in the middle half of OBB i.  Returns a dict of arrays, one
    row per state: p, axis, top (1: g1), obb, d, ulps (d in double ulps of g), and the partner
    end e of the face-parallel edge p -> e (e[k] == p[k], up to 0.3 m along the OBB's longest
    other axis towards its centre, inside the inflated OBB)."""
    _, ref = world(name)
    g0, g1 = bounds(name)
    rs = np.random.RandomState(5)
    rows = []
    for k in range(3):
        for top in (1, 0):
            i = int(np.argmax(ref["aabb_hi"][:, k]) if top else np.argmin(ref["aabb_lo"][:, k]))
            o = ref[i]
            g = g1[k] if top else g0[k]
            assert k == 2 or (o["rot"][0] == 1.0 and i >= len(ref) - len(CAPS))
            ulp = np.spacing(abs(g)) if g != 0 else np.spacing(1.0)
            s = float(np.spacing(np.float32(abs(g)))) if g != 0 else float(np.spacing(np.float32(1.0)))
            ds = [u * ulp for u in ULP_RUNGS] + [s * 2.0 ** -j for j in range(POW_RUNGS)]
            others = [a for a in range(3) if a != k]
            m = max(others, key=lambda a: o["half"][a])  # the parallel edge runs along local axis m
            r = ro_of(o)
            for d in ds:
                for _ in range(LADDER_REPS):
                    l = rs.uniform(-0.5, 0.5, 3) * o["half"]
                    l[k] = 0.0
                    p = _local_to_world(o, l)
                    p[k] = g - d if top else g + d
                    l2 = l.copy()
                    step = min(0.3, o["half"][m] + r)
                    l2[m] = l[m] - (1.0 if l[m] >= 0 else -1.0) * step
                    e = _local_to_world(o, l2)
                    e[k] = p[k]
                    rows.append((p, k, top, i, d, d / ulp, e))
    out = {"p": np.array([r[0] for r in rows]), "axis": np.array([r[1] for r in rows]),
           "top": np.array([r[2] for r in rows]), "obb": np.array([r[3] for r in rows]),
           "d": np.array([r[4] for r in rows]), "ulps": np.array([r[5] for r in rows]),
           "e": np.array([r[6] for r in rows])}
    _frozen(*out.values())
    return out


def ro_of(o):
    _, rg, ro = setup()
    return rg if o["is_gate"] else ro


def float_image_points(ref):
    """Per OBB and AABB face: states whose coordinate is float64(float32(face)) and 1 and 2
    double ulps to either side of it (states that share the face's float image), the other
    coordinates at the AABB's centre."""
    pts = []
    for o in ref:
        mid = (o["aabb_lo"] + o["aabb_hi"]) / 2
        for k in range(3):
            for v in (o["aabb_lo"][k], o["aabb_hi"][k]):
                img = np.float64(np.float32(v))
                for u in (-2, -1, 0, 1, 2):
                    p = mid.copy()
                    p[k] = _nudged(img, u)
                    pts.append(p)
    return np.array(pts)


@functools.lru_cache(maxsize=None)
def states(name):
    """(N_STATES states, kind per state), shuffled so that every prefix holds some of each kind:
    0 uniform (in the bounds widened by 1 m, and in single AABBs widened by 0.1 m), 1 adversarial_points (on and an ulp around every AABB
    face, on the OBB thresholds), 2 ladder, 3 float images of the faces, 4 NaN / inf / 1e30."""
    _, ref = world(name)
    g0, g1 = bounds(name)
    c = (g0 + g1) / 2
    odd = np.array([[np.nan, c[1], c[2]], [c[0], np.nan, c[2]], [np.nan] * 3, [np.inf, c[1], c[2]],
                    [c[0], -np.inf, c[2]], [np.inf, np.inf, np.inf], [-np.inf, -np.inf, -np.inf],
                    [1e30, c[1], c[2]], [c[0], -1e30, c[2]], [1e30, 1e30, 1e30], [c[0], c[1], 1e30]])
    parts = [None, adversarial_points(ref), ladder(name)["p"], float_image_points(ref), odd]
    n_uni = N_STATES - sum(len(p) for p in parts[1:])
    assert n_uni >= 2000, n_uni
    # (the world is sparse: of states uniform over the whole box 99 % are valid, so half of the
    # uniform states are drawn over the box and half over the AABB, widened by 0.1 m, of an OBB
    # each, the OBBs taken in turn)
    n_box = n_uni // 2
    u = synth.sample_states(32, np.zeros(3), np.ones(3), n_uni - n_box)
    own = np.arange(n_uni - n_box) % len(ref)
    lo, hi = ref["aabb_lo"][own] - 0.1, ref["aabb_hi"][own] + 0.1
    parts[0] = np.vstack([synth.sample_states(31, g0 - 1.0, g1 + 1.0, n_box), lo + (hi - lo) * u])
    kind = np.concatenate([np.full(len(p), j, np.int8) for j, p in enumerate(parts)])
    lad = np.concatenate([np.full(len(p), -1, np.int64) if j != 2 else np.arange(len(p)) for j, p in enumerate(parts)])
    perm = np.random.RandomState(17).permutation(N_STATES)
    pts = np.ascontiguousarray(np.vstack(parts)[perm])
    assert pts.shape == (N_STATES, 3) and N_STATES % 4 == 3
    return _frozen(pts, kind[perm], lad[perm])  # lad: the state's row in ladder(name), or -1


@functools.lru_cache(maxsize=None)
def edges(name):
    """(s, e, kind) of N_EDGES edges, shuffled: 0 synth.edges in the bounds, 1 the ladder states as
    degenerate edges (s == e), 2 the face-parallel ladder edges (every discrete32 sample
    s + (e - s) t has exactly the ladder state's p[k]), 3 edges that cross a face of the union
    from outside into the OBB that attains it."""
    _, ref = world(name)
    g0, g1 = bounds(name)
    L = ladder(name)
    rs = np.random.RandomState(23)
    cs, ce = [], []
    for k in range(3):
        for top in (1, 0):
            sel = np.flatnonzero((L["axis"] == k) & (L["top"] == top))
            o = ref[int(L["obb"][sel[0]])]
            g = g1[k] if top else g0[k]
            for _ in range(16):
                l = rs.uniform(-0.5, 0.5, 3) * o["half"]
                l[k] = 0.0
                a = _local_to_world(o, l)
                b = a.copy()
                sign = 1.0 if top else -1.0
                a[k] = g + sign * rs.uniform(0.01, 0.3)
                b[k] = g - sign * rs.uniform(0.01, 0.2)
                cs.append(a)
                ce.append(b)
    s_parts = [None, L["p"], L["p"], np.array(cs)]
    e_parts = [None, L["p"], L["e"], np.array(ce)]
    n_rand = N_EDGES - sum(len(p) for p in s_parts[1:])
    assert n_rand >= 1500, n_rand
    s_parts[0], e_parts[0] = synth.edges(33, 34, g0, g1, n_rand, max_len=1.5)
    kind = np.concatenate([np.full(len(p), j, np.int8) for j, p in enumerate(s_parts)])
    perm = np.random.RandomState(19).permutation(N_EDGES)
    s = np.ascontiguousarray(np.vstack(s_parts)[perm])
    e = np.ascontiguousarray(np.vstack(e_parts)[perm])
    assert s.shape == (N_EDGES, 3) and N_EDGES % 4 == 3
    return _frozen(s, e, kind[perm])


@functools.lru_cache(maxsize=None)
def hover_points(name):
    """(points, is_ladder): every ladder state and 200 of adversarial_points."""
    _, ref = world(name)
    adv = adversarial_points(ref)
    adv = adv[np.sort(np.random.RandomState(29).choice(len(adv), 200, replace=False))]
    lad = ladder(name)["p"]
    return _frozen(np.ascontiguousarray(np.vstack([lad, adv])),
                   np.concatenate([np.ones(len(lad), bool), np.zeros(len(adv), bool)]))


def hover_tracks(name):
    """One one-segment track of T_HOVER seconds per hover point, in the layout capi.minsnap_batch
    returns: every coefficient zero except the constant term, which is the point.  Every sampled
    row is then that point exactly, whatever the evaluation order."""
    pts, _ = hover_points(name)
    Ts = [np.array([T_HOVER]) for _ in pts]
    Cs = []
    for p in pts:
        c = np.zeros((1, 3, 10))
        c[0, :, 0] = p
        Cs.append(c)
    return Ts, Cs


# ---- the oracle's answers (computed once, shared, read-only) -------------------------------------
@functools.lru_cache(maxsize=None)
def exp_states(name, variant):
    """variant: 0 / 1 = can_pass_gate, else a min_distance."""
    _, rg, ro = setup()
    _, ref = world(name)
    pts = states(name)[0]
    if variant in (0, 1):
        return _frozen(O.check_states(ref, rg, ro, pts, bool(variant), threads=8))
    return _frozen(O.check_states_mindist(ref, pts, float(variant)))


@functools.lru_cache(maxsize=None)
def exp_motions(name, mode, can_pass):
    _, rg, ro = setup()
    _, ref = world(name)
    s, e, _ = edges(name)
    return _frozen(O.check_motions(ref, rg, ro, s, e, bool(can_pass), mode, threads=8))


@functools.lru_cache(maxsize=None)
def exp_hover_mindist(name, md):
    _, ref = world(name)
    return _frozen(O.check_states_mindist(ref, hover_points(name)[0], md))


@functools.lru_cache(maxsize=None)
def exp_hover_chords(name, can_pass):
    _, rg, ro = setup()
    _, ref = world(name)
    p = hover_points(name)[0]
    return _frozen(O.check_motions(ref, rg, ro, p, p, bool(can_pass), 0, threads=8))


def sliver_width(name, k):
    """The width in metres of the band below g1[k] whose fine coordinate exceeds old_limit: the
    largest ladder rung d on the +k face with fine_coord(g1[k] - d) > 4 n (1 + 2^-20); 0.0 if none."""
    obbs, _ = world(name)
    g = cull_grid(obbs)
    L = ladder(name)
    sel = (L["axis"] == k) & (L["top"] == 1)
    f = fine_coord(L["p"][sel, k], g["of"][k], g["i4"][k])
    over = f > old_limit(g["n"][k])
    return float(L["d"][sel][over].max()) if over.any() else 0.0
