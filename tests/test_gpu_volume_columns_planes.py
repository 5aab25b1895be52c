"""The column calls where their bit-plane counters reach the high planes (csrc/vrc_columns.hip: first, last, count and runs of
the profile, P - lo and P - hi of the select), at the depths 7 .. 10 whose column lengths first put a one into the planes 6 .. 9
of a coordinate or a run count and into plane 10 of a count.  The scenes are tests/columns_cases.py's: a catalogue of column
programs -- combs, single runs, pairs of voxels and runs on word seams, around every power of two -- dealt over bundles so that
the 16 (4) columns that share a lane's registers differ in their high planes.  Every expected value follows from the run lists
(tests/test_volume_columns_cases_host.py holds them to columns_model and says which wrong kernels they catch); nothing is
derived from a device result.  The scenes are built with fillBoxes, one box a run.  Above 128^3 nothing dense comes down:
records are compared one by one, and a volume by solidCount() plus countBoxes() over the expected spans -- every expected
voxel is there and there are no others."""
import numpy as np
import pytest

import columns_cases as cc
import columns_model as model

pytestmark = pytest.mark.gpu

KINDS = (model.SOLID, model.EMPTY, model.BOTH)
I32 = np.iinfo(np.int32)


def volume_of_scene(sc):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(sc.depth)
    volume.fillBoxes(sc.boxes())
    assert volume.solidCount() == sc.solid()
    return volume


def record_diff(got, want):
    bad = np.argwhere(got != want)
    return len(bad), [(tuple(i), tuple(got[tuple(i)]), tuple(want[tuple(i)])) for i in bad[:3].tolist()]


def holds_exactly(volume, boxes, sizes):
    """the volume's solid voxels are those of the disjoint boxes, all of them: (ok, what was counted)"""
    counted = volume.countBoxes(boxes) if len(boxes) else np.zeros(0, np.uint64)
    total = volume.solidCount()
    return bool(np.array_equal(counted, sizes) and total == int(sizes.sum())), (total, int(sizes.sum()), int((counted != sizes).sum()))


def kind_of(i, lo):
    """the kinds in turn; EMPTY and BOTH only with lo >= 1, where the empty columns (P = 0 everywhere) select nothing"""
    return KINDS[i % 3] if lo >= 1 else model.SOLID


# ---- 1. profile ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("depth", [7, 8, 9, 10])
def test_profile_of_programmed_columns(built, depth, axis):
    """small rects around every programmed bundle, which cut it on every side, and the whole face; then the same voxels met
    along the other four directions, the whole face"""
    sc = cc.scene(depth, axis)
    S = sc.S
    volume = volume_of_scene(sc)
    for side in (0, 1):
        direction = 2 * axis + side
        for a, b in sc.placed:
            for rect in cc.rects_around(axis, S, a, b):
                got, want = volume.columnProfile(direction, rect), sc.profile(side, rect)
                assert got.shape == want.shape and np.array_equal(got, want), (depth, direction, (a, b), rect, record_diff(got, want))
        got, want = volume.columnProfile(direction), sc.profile(side)
        assert np.array_equal(got, want), (depth, direction, record_diff(got, want))
    for other in range(3):
        if other != axis:
            across = sc.seen_along(other)
            for side in (0, 1):
                got, want = volume.columnProfile(2 * other + side), across.profile(side)
                assert np.array_equal(got, want), (depth, axis, 2 * other + side, record_diff(got, want))
    assert volume.solidCount() == sc.solid()                                   # the volume is only read
    volume.close()


@pytest.mark.parametrize("axis", range(3))
def test_maps_of_programmed_columns(built, axis):
    """heightMap, thicknessMap and isHeightField at depth 9, from the same records; then without the columns of several runs
    (cleared with boxes), which leaves a height field, and without the runs that float, which leaves a grounded one"""
    sc = cc.scene(9, axis)
    S = sc.S
    volume = volume_of_scene(sc)
    for side in (0, 1):
        direction = 2 * axis + side
        p = sc.profile(side)
        want = np.where(p["count"] > 0, p["first"].astype(np.int64), -5).astype(np.int32)
        assert np.array_equal(volume.heightMap(direction, -5), want), (axis, side)
        assert (p["runs"] > 1).any() and volume.isHeightField(direction) is False and volume.isHeightField(direction, grounded=True) is False
    assert np.array_equal(volume.thicknessMap(axis), sc.profile(0)["count"])
    assert int(volume.thicknessMap(axis).sum(dtype=np.uint64)) == sc.solid()
    volume.fillBoxes([cc.box_of(axis, u, v, 0, S) for u, v, runs in sc.columns if len(runs) > 1], False)
    single = [(u, v, runs) for u, v, runs in sc.columns if len(runs) == 1]
    assert volume.solidCount() == sum(runs[0][1] - runs[0][0] for _, _, runs in single)
    for side in (0, 1):
        direction = 2 * axis + side
        floating = [cc.box_of(axis, u, v, 0, S) for u, v, runs in single if (runs[0][1] != S if side else runs[0][0] != 0)]
        assert 0 < len(floating) < len(single)
        assert volume.isHeightField(direction) is True and volume.isHeightField(direction, grounded=True) is False
        grounded = volume.clone()
        grounded.fillBoxes(floating, False)
        assert grounded.solidCount() > 0 and grounded.isHeightField(direction, grounded=True) is True
        grounded.close()
    volume.close()


# ---- 2. select ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("depth", [8, 9, 10])
def test_select_bands_around_the_powers_of_two(built, depth, axis):
    """every band of columns_cases.bands in both directions of the axis, REPLACE into what the band before left (once into a
    slab that lies outside every expected span), and one ANDNOT from a full volume"""
    import cpuvoxelraycaster_amd as vrc
    sc = cc.scene(depth, axis)
    S = sc.S
    src, dst = volume_of_scene(sc), vrc.VoxelVolume(depth)
    dst.fillBoxes([cc.box_of_rect(axis, (0, 0, S, 3), 0, S), cc.box_of_rect(axis, (0, 0, S, S), S // 2, S // 2 + 1)])
    assert dst.solidCount() == 3 * S * S + S * S - 3 * S
    for side in (0, 1):
        direction = 2 * axis + side
        for i, (lo, hi) in enumerate(cc.bands(S)):
            of = kind_of(i + side, lo)
            assert src.selectColumns(direction, lo, hi, of, dst) is dst
            boxes, sizes = sc.selection_boxes(side, lo, hi, of)
            ok, counted = holds_exactly(dst, boxes, sizes)
            assert ok, (depth, direction, lo, hi, of, counted)
    lo, hi = S // 4 - 1, S // 2 + 1
    for side, of in ((0, model.BOTH), (1, model.SOLID)):
        dst.fillBoxes([[0, 0, 0, S, S, S]])
        src.selectColumns(2 * axis + side, lo, hi, of, dst, model.ANDNOT)
        boxes, sizes = sc.selection_boxes(side, lo, hi, of)
        assert sizes.sum() > 0 and not dst.countBoxes(boxes).any() and dst.solidCount() == S ** 3 - int(sizes.sum()), (depth, axis, side)
    assert src.solidCount() == sc.solid()
    src.close()
    dst.close()


# ---- 3. fill ------------------------------------------------------------------------------------------------------------

def fill_maps(S, shape):
    """lo and hi maps from the values around every power of two, -1, S, S + 1 and the ends of int32, dealt so that a column
    differs from every other one of its bundle (2 x 8 or 2 x 2 columns): the index into the values moves by 11 along u and by 1
    along v, and there are more than 18 values"""
    values = np.array(list(dict.fromkeys(cc.band_values(S) + [-1, S, S + 1, I32.min, I32.max])), np.int64)
    i, j = np.indices(shape)
    assert len(values) > 11 + 7
    return values[(11 * i + j) % len(values)].astype(np.int32), values[(5 * i + 13 * j + 5) % len(values)].astype(np.int32)


def fill_case(S, axis):
    rect = (S - 47, S - 45, S - 6, S - 4)                                      # odd bounds, 41 x 41, high up in both face coordinates
    lo_map, hi_map = fill_maps(S, (rect[2] - rect[0], rect[3] - rect[1]))
    lo, hi = np.clip(lo_map.astype(np.int64), 0, S), np.clip(hi_map.astype(np.int64), 0, S)
    u, v = np.nonzero(lo < hi)
    boxes = np.array([cc.box_of(axis, rect[0] + int(a), rect[1] + int(b), int(lo[a, b]), int(hi[a, b])) for a, b in zip(u, v)], np.uint32)
    return rect, lo_map, hi_map, boxes, (hi - lo)[u, v].astype(np.uint64)


@pytest.mark.parametrize("axis", range(3))
def test_fill_maps_around_the_powers_of_two(built, axis):
    import cpuvoxelraycaster_amd as vrc
    S = 512
    rect, lo_map, hi_map, boxes, sizes = fill_case(S, axis)
    n = int(sizes.sum())
    columns = cc.box_of_rect(axis, rect, 0, S)
    assert len(boxes) > 600 and sizes.max() == S and sizes.min() == 1
    # OR into an empty volume
    volume = vrc.VoxelVolume(9)
    volume.fillColumns(axis, lo_map, hi_map, rect, model.OR)
    ok, counted = holds_exactly(volume, boxes, sizes)
    assert ok, (axis, "or", counted)
    # REPLACE over a block that covers a part of the rect and lies partly outside it: the rect's columns hold the spans alone
    u0, v0, u1, v1 = S - 30, S - 60, S, S - 20
    block = cc.box_of_rect(axis, (u0, v0, u1, v1), 100, 400)
    outside = 300 * ((u1 - u0) * (v1 - v0) - (min(u1, rect[2]) - max(u0, rect[0])) * (min(v1, rect[3]) - max(v0, rect[1])))
    volume.fillBoxes([[0, 0, 0, S, S, S]], False)
    volume.fillBoxes([block])
    volume.fillColumns(axis, lo_map, hi_map, rect, model.REPLACE)
    assert np.array_equal(volume.countBoxes(boxes), sizes) and volume.countBoxes([columns]).tolist() == [n], (axis, "replace")
    assert volume.solidCount() == n + outside and outside > 0, (axis, "replace")
    # ANDNOT from a full volume, by the complement
    volume.fillBoxes([[0, 0, 0, S, S, S]])
    volume.fillColumns(axis, lo_map, hi_map, rect, model.ANDNOT)
    assert not volume.countBoxes(boxes).any() and volume.countBoxes([columns]).tolist() == [41 * 41 * S - n], (axis, "andnot")
    assert volume.solidCount() == S ** 3 - n, (axis, "andnot")
    volume.close()


# ---- 4. the bridge: the same scenes, dense, at depth 7 ---------------------------------------------------------------------

@pytest.mark.parametrize("axis", range(3))
def test_dense_comparison_at_depth_7(built, axis):
    """the device, columns_model on the dense scene and the sparse model agree at once"""
    import cpuvoxelraycaster_amd as vrc
    sc = cc.scene(7, axis)
    S = sc.S
    vol = sc.dense()
    src, dst = volume_of_scene(sc), vrc.VoxelVolume(7)
    assert np.array_equal(src.download(), vol)
    for side in (0, 1):
        direction = 2 * axis + side
        got, dense, sparse = src.columnProfile(direction), model.profile(vol, direction), sc.profile(side)
        assert np.array_equal(dense, sparse) and np.array_equal(got, dense), (direction, record_diff(got, dense))
        for i, (lo, hi) in enumerate(cc.bands(S)[side::3]):
            of = kind_of(i, lo)
            src.selectColumns(direction, lo, hi, of, dst)
            got, dense = dst.download(), model.selection(vol, direction, lo, hi, of)
            assert np.array_equal(dense, sc.selection_scene(side, lo, hi, of).dense()) and np.array_equal(got, dense), (direction, lo, hi, of)
            boxes, sizes = sc.selection_boxes(side, lo, hi, of)
            assert holds_exactly(dst, boxes, sizes)[0]                         # the exactness check of the larger depths, on the same result
    rect, lo_map, hi_map, boxes, sizes = fill_case(S, axis)
    for op in (model.REPLACE, model.OR, model.ANDNOT):
        volume = src.clone()
        volume.fillColumns(axis, lo_map, hi_map, rect, op)
        assert np.array_equal(volume.download(), model.fill(vol, axis, lo_map, hi_map, rect, op)), (axis, op)
        volume.close()
    dst.fillBoxes([[0, 0, 0, S, S, S]], False)
    dst.fillColumns(axis, lo_map, hi_map, rect, model.OR)
    assert holds_exactly(dst, boxes, sizes)[0]
    src.close()
    dst.close()
