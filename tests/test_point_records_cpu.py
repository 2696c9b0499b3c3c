"""Host index build (no GPU): the 128-byte point records the plain point test of
k_states_v5 reads, and the filling flag in bit 15 of the candidate-list ids.

For the filling world of point_record_inputs (gate frames, filling openings and obstacles,
each kind rotated and unrotated) and the C2 world: every point record equals, bit for bit,
what the 17-double record and the world's two radii imply -- AABB, centre, cos / sin copied,
t = filling ? h : h + r computed in numpy float64 (one IEEE addition, as the kernel did per
pair) -- and every list id carries its OBB's filling flag with the id itself unchanged.
"""
import numpy as np
import pytest

import point_record_inputs as P

F_HX, R_META = 11, 16


@pytest.mark.parametrize("name", ["filling", "c2"])
def test_point_records_match_aos_records(name):
    _, rg, ro = P.setup(name)
    obbs, _ = P.world(name)
    recs, pt, _, layout = P.point_records(obbs, rg, ro)
    n = len(obbs)
    meta = recs[:, R_META].copy().view(np.uint64)
    fill, gate = (meta & 1) != 0, (meta & 2) != 0
    assert np.array_equal(fill, obbs["filling"] != 0) and np.array_equal(gate, obbs["is_gate"] != 0)
    if name == "filling":  # every kind, rotated and unrotated
        unrot = obbs["rot"][:, 3] == 0.0
        for kind in (fill, gate & ~fill, ~gate):
            assert (kind & unrot).any() and (kind & ~unrot).any()
    else:
        assert not fill.any()
    # fields F_LOX .. F_SIN: copied
    assert np.array_equal(pt[:, :F_HX].view(np.uint64), recs[:, :F_HX].view(np.uint64))
    # thresholds: h for a filling OBB, else h + r in float64
    h = recs[:, F_HX:F_HX + 3]
    r = np.where(gate, np.float64(rg), np.float64(ro))[:, None]
    t = np.where(fill[:, None], h, h + r)
    assert np.array_equal(np.ascontiguousarray(pt[:, F_HX:F_HX + 3]).view(np.uint64),
                          np.ascontiguousarray(t).view(np.uint64))
    assert np.array_equal(t, P.thresholds(obbs, rg, ro))
    assert not pt[:, 14:].any()  # the spare doubles
    # layout: 17-double records, then 128-byte point records (16-byte aligned), then the lists
    assert layout["pt"] % 16 == 0 and 0 <= layout["pt"] - (layout["aos"] + 136 * n) < 16
    assert layout["lists"] == layout["pt"] + 128 * n and layout["ids"] > layout["lists"]


@pytest.mark.parametrize("name", ["filling", "c2"])
def test_list_ids_carry_the_filling_flag(name):
    _, rg, ro = P.setup(name)
    obbs, _ = P.world(name)
    _, _, ids, layout = P.point_records(obbs, rg, ro)
    assert layout["id_mask"] == 0x7FFF and len(ids) > len(obbs)
    low = ids & 0x7FFF
    assert low.max() < len(obbs)
    assert np.array_equal(np.unique(low), np.arange(len(obbs)))  # every OBB is some cell's candidate
    assert np.array_equal((ids >> 15) != 0, obbs["filling"][low] != 0)
    if name == "filling":
        assert 0 < int((ids >> 15).sum()) < len(ids)
