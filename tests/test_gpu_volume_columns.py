"""The column calls on the device (include/vrc.h: vrc_columns_profile, vrc_columns_fill, vrc_columns_select) against the numpy
model of columns_model.py, bit for bit.  The sizes are the smallest at which each hazard of csrc/vrc_columns.hip first appears:
  4^3    two brick rows share a word: the walk takes a half as a word (shift and mask), a column along z is half a word, the
         fill and the select store the half with atomics; the walks along x and y have two steps;
  8^3    one word per row along z, no carry; every word whole;
  16^3   the first carry from word to word along z (along x and y every size carries);
  32^3   rects that cut bricks and words on every side with whole words between them;
  64^3   more bundles than one 64-lane workgroup for every axis (x, y: 256; z: 1024); the fill's launch has several groups;
  128^3  walks of 64 (x, y) and 16 (z) words, rows of 16 words in the fill.
A lane takes one bundle and the launches are not capped, so no size makes a lane take a second item, and no state crosses
lanes.  What still grows with the size is the counters: plane b of a count first holds a one at a count of 2^b.  A full
volume at 256^3 reaches plane 8; planes 9 and 10 are reached at 512^3 and 1024^3 only, so one case runs there on a full
volume and checks records of a small rect and counts of boxes -- nothing dense comes down at that size.  "Reached" is all a
full volume does: its first and last are 0 or S - 1, its count S or S - 1 and its runs 1 or 2, so every plane is all ones or
all zeros.  tests/test_gpu_volume_columns_planes.py runs columns with mixed patterns in the high planes of all four
numbers and of the select's two, at the depths 7 .. 10 (the cases are tests/columns_cases.py's)."""
import numpy as np
import pytest

import cells_model
import columns_model as model
from volume_support import Stream, committed, same, terrain_volume, volume_of

pytestmark = pytest.mark.gpu

SIZES = [4, 8, 16, 32]
OPS = (model.REPLACE, model.OR, model.ANDNOT)


def depth_of(S):
    return S.bit_length() - 1


def rects(S):
    """the whole face; odd bounds that cut bricks and words; even bounds; one column"""
    return [None, (1, 1, S - 1, S), (0, 2, S - 2, S), (S // 2 + 1, S - 1, S // 2 + 2, S)]


def fields(S):
    rng = np.random.default_rng(100 + S)
    out = {"empty": np.zeros((S, S, S), np.uint8), "full": np.ones((S, S, S), np.uint8), "bands": cells_model.three_band(S),
           "random": (rng.random((S, S, S)) < 0.5).astype(np.uint8)}
    for axis in range(3):
        out["alternating%d" % axis] = model.alternating(S, axis, axis & 1)
    return out


def differing(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:4].tolist()


def record_diff(got, want):
    bad = np.argwhere(got != want)
    return len(bad), [(tuple(i), tuple(got[tuple(i)]), tuple(want[tuple(i)])) for i in bad[:3].tolist()]


# ---- 1. profile ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", SIZES)
def test_profile_fields_and_rects(built, S):
    from cpuvoxelraycaster_amd import capi
    for name, vol in fields(S).items():
        volume = volume_of(vol, depth_of(S))
        scratch = volume.editScratchBytes()
        for direction in model.DIRECTIONS:
            whole = model.profile(vol, direction)
            if name.startswith("alternating") and direction >> 1 == int(name[-1]):
                assert (whole["runs"] == S // 2).all()
            for rect in rects(S):
                got = volume.columnProfile(direction, rect)
                want = model.profile(vol, direction, rect)
                assert got.dtype == capi.COLUMN_DTYPE and got.shape == want.shape
                assert np.array_equal(got, want), (S, name, direction, rect, record_diff(got, want))
        assert volume.editScratchBytes() == scratch                   # the records are staged in a block of the call's own
        assert np.array_equal(volume.download(), vol)
        volume.close()


def single_voxel_cases(S):
    if S <= 8:
        return [tuple(p) for p in np.indices((S, S, S)).reshape(3, -1).T.tolist()]
    e = S - 1
    rng = np.random.default_rng(S)
    corners = [(x, y, z) for x in (0, e) for y in (0, e) for z in (0, e)]
    seams = [tuple(int(c) for c in rng.permutation([a, b, int(rng.integers(0, S))])) for a in (7, 8) for b in (0, 1, 7, 8, e)]
    return corners + seams + [tuple(p) for p in rng.integers(0, S, (200, 3)).tolist()]


@pytest.mark.parametrize("S", SIZES)
def test_profile_one_voxel_at_every_position(built, S):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(depth_of(S))
    for p in single_voxel_cases(S):
        volume.setVoxels([p])
        for direction in model.DIRECTIONS:
            axis = direction >> 1
            u, v = [p[a] for a in range(3) if a != axis]
            want = np.zeros((S, S), model.COLUMN_DTYPE)
            want["first"] = want["last"] = model.NONE
            want[u, v] = (p[axis], p[axis], 1, 1)
            got = volume.columnProfile(direction)
            assert np.array_equal(got, want), (S, p, direction, record_diff(got, want))
        volume.setVoxels([p], False)
    assert volume.solidCount() == 0
    volume.close()


def test_profile_in_device_memory_behind_an_edit(built):
    """the records go into a window of a larger, pre-filled device buffer; the call runs on the edit's stream and on another
    one, both behind the asynchronous edit"""
    import torch
    S = 32
    rng = np.random.default_rng(32)
    base = (rng.random((S, S, S)) < 0.2).astype(np.uint8)
    extra = rng.integers(0, S, (3000, 3)).astype(np.uint32)
    edited = base.copy()
    edited[tuple(extra.T.astype(np.int64))] = 1
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    for other_stream in (False, True):
        for direction, rect in [(2, None), (5, (3, 5, 30, 18)), (1, (7, 0, 8, 32))]:
            want = model.profile(edited, direction, rect)
            assert not np.array_equal(want, model.profile(base, direction, rect))
            n = want.size
            buf = torch.full((n + 8, 4), 0x7B7B7B7B, dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            volume = volume_of(base, 5)
            with Stream() as stream, Stream() as second:
                volume.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
                volume.columnProfileDevice(direction, buf.data_ptr() + 4 * 16, rect, second if other_stream else stream)
            got = buf.cpu().numpy().view(np.uint32)
            assert (got[:4] == 0x7B7B7B7B).all() and (got[4 + n:] == 0x7B7B7B7B).all()       # nothing outside the window
            records = got[4:4 + n].copy().view(model.COLUMN_DTYPE).reshape(want.shape)
            assert np.array_equal(records, want), (other_stream, direction, rect, record_diff(records, want))
            on_device = volume.columnProfile(direction, rect, device=True)
            assert np.array_equal(on_device.cpu().numpy().view(np.uint32).reshape(-1, 4), got[4:4 + n])
            volume.close()


# ---- 2. fill ------------------------------------------------------------------------------------------------------------

def random_maps(rng, shape, S):
    """int32 maps with negatives, values above S, the ends of int32 and lo >= hi"""
    I = np.iinfo(np.int32)
    out = []
    for _ in range(2):
        m = rng.integers(-3, S + 4, shape).astype(np.int32)
        kind = rng.integers(0, 10, shape)
        m[kind == 0], m[kind == 1] = I.min, I.max
        out.append(m)
    if out[0].size >= 4:
        # whatever the draw: a span that starts below 0 and ends above S, an empty one, and the ends of int32 both ways round
        out[0].flat[:4], out[1].flat[:4] = (-2, 5, I.min, I.max), (S + 3, 5, I.max, I.min)
    return out


@pytest.mark.parametrize("S", SIZES)
def test_fill_maps_constants_ops_and_rects(built, S):
    import torch
    rng = np.random.default_rng(200 + S)
    base = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    source = volume_of(base, depth_of(S))
    scratch = None
    for axis in range(3):
        for rect in rects(S):
            shape = (S, S) if rect is None else (rect[2] - rect[0], rect[3] - rect[1])
            lo_map, hi_map = random_maps(rng, shape, S)
            for op in OPS:
                for which in range(4):
                    lo = lo_map if which & 1 else int(rng.integers(-1, S // 2 + 1))
                    hi = hi_map if which & 2 else int(rng.integers(S // 2, S + 2))
                    volume = source.clone()
                    scratch = volume.editScratchBytes() if scratch is None else scratch
                    if which == 3 and op == model.OR:
                        # the maps in device memory, asynchronous
                        t_lo, t_hi = torch.from_numpy(lo_map).cuda(), torch.from_numpy(hi_map).cuda()
                        torch.cuda.synchronize()
                        volume.fillColumnsDevice(axis, t_lo.data_ptr(), 0, t_hi.data_ptr(), 0, rect, op)
                    else:
                        assert volume.fillColumns(axis, lo, hi, rect, op) is volume
                    got, want = volume.download(), model.fill(base, axis, lo, hi, rect, op)
                    assert np.array_equal(got, want), (S, axis, rect, op, which, differing(got, want))
                    assert volume.editScratchBytes() == scratch       # the maps are staged in a block of the call's own
                    volume.close()
    assert np.array_equal(source.download(), base)
    source.close()


# ---- 3. select ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", SIZES)
def test_select_bands_kinds_and_ops(built, S):
    import cpuvoxelraycaster_amd as vrc
    rng = np.random.default_rng(300 + S)
    before = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    whole = ((0, 0, 0), (S, S, S), (0, 0, 0))
    prefilled, dst = volume_of(before, depth_of(S)), vrc.VoxelVolume(depth_of(S))
    for name, vol in fields(S).items():
        src = volume_of(vol, depth_of(S))
        for direction in model.DIRECTIONS:
            k = int(rng.integers(1, S + 1))
            lo = int(rng.integers(0, S + 2))
            bands = [(0, 1), (0, k), (k, S + 1), (k, k), (lo, int(rng.integers(lo, S + 2))), (1, 0xFFFFFFFF)]
            for of in (model.SOLID, model.EMPTY, model.BOTH):
                for op in OPS:
                    for lo_hi in bands:
                        dst.copyRegion(prefilled, *whole)
                        assert src.selectColumns(direction, *lo_hi, of, dst, op) is dst
                        got, want = dst.download(), model.select(before, vol, direction, *lo_hi, of, op)
                        assert np.array_equal(got, want), (S, name, direction, lo_hi, of, op, differing(got, want))
        assert np.array_equal(src.download(), vol)                     # the source is only read
        src.close()
    prefilled.close()
    dst.close()


@pytest.mark.parametrize("S", SIZES)
def test_lit_surface_is_the_profiles_first(built, S):
    for name, vol in fields(S).items():
        src = volume_of(vol, depth_of(S))
        for direction in model.DIRECTIONS:
            axis = direction >> 1
            lit = src.skyLit(direction)
            got = np.moveaxis(lit.download(), axis, -1)
            lit.close()
            p = src.columnProfile(direction)
            assert np.array_equal(got.sum(-1), p["count"] > 0), (S, name, direction)          # one voxel per non-empty column
            u, v = np.nonzero(p["count"])
            assert got[u, v, p["first"][u, v]].all(), (S, name, direction)                     # at the profile's first
        top, cave = src.topLayers(3, 2), src.sheltered(3)
        assert np.array_equal(top.download(), model.selection(vol, 3, 0, 2, model.SOLID))
        assert np.array_equal(cave.download(), model.selection(vol, 3, 1, S + 1, model.EMPTY))
        for thing in (top, cave, src):
            thing.close()


# ---- 4. round trips -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", SIZES)
def test_profile_then_fill_reproduces_a_single_run_field(built, S):
    import cpuvoxelraycaster_amd as vrc
    rng = np.random.default_rng(400 + S)
    for axis in range(3):
        lo, hi = rng.integers(-2, S + 3, (2, S, S))
        vol = model.fill(np.zeros((S, S, S), np.uint8), axis, lo, hi)
        volume = volume_of(vol, depth_of(S))
        assert int(volume.thicknessMap(axis).sum(dtype=np.uint64)) == volume.solidCount() == int(vol.sum())
        for direction in (2 * axis, 2 * axis + 1):
            p = volume.columnProfile(direction)
            assert (p["runs"] <= 1).all() and volume.isHeightField(direction)
            least, greatest = np.minimum(p["first"], p["last"]).astype(np.int64), np.maximum(p["first"], p["last"]).astype(np.int64)
            least[p["count"] == 0] = greatest[p["count"] == 0] = -1            # NONE: an empty span
            again = vrc.VoxelVolume(depth_of(S))
            again.fillBoxes([[0, 0, 0, S, S, 1]])                                # REPLACE clears it
            again.fillColumns(axis, least.astype(np.int32), (greatest + 1).astype(np.int32), None, model.REPLACE)
            assert np.array_equal(again.download(), vol), (S, direction)
            again.close()
        volume.close()


# ---- 5. larger volumes: many workgroups, long walks ------------------------------------------------------------------------

@pytest.mark.parametrize("S", [64, 128])
def test_larger_volume(built, S):
    import cpuvoxelraycaster_amd as vrc
    depth = depth_of(S)
    rng = np.random.default_rng(S)
    src, dst = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
    src.fillRandom(19, 0.4)
    vol = cells_model.random_set(19, cells_model.threshold_of(0.4), S)
    rect = (5, 3, S - 9, S - 1)
    for direction in model.DIRECTIONS:
        got, want = src.columnProfile(direction), model.profile(vol, direction)
        assert np.array_equal(got, want), (S, direction, record_diff(got, want))
        got, want = src.columnProfile(direction, rect), model.profile(vol, direction, rect)
        assert np.array_equal(got, want), (S, direction, rect, record_diff(got, want))
        lo = int(rng.integers(0, 5))
        hi = lo + int(rng.integers(1, S // 3))
        src.selectColumns(direction, lo, hi, 1 + direction % 3, dst)
        got, want = dst.download(), model.selection(vol, direction, lo, hi, 1 + direction % 3)
        assert np.array_equal(got, want), (S, direction, lo, hi, differing(got, want))
    for axis, op in zip(range(3), OPS):
        shape = (rect[2] - rect[0], rect[3] - rect[1])
        lo_map, hi_map = random_maps(rng, shape, S)
        volume = src.clone()
        volume.fillColumns(axis, lo_map, hi_map, rect, op)
        got, want = volume.download(), model.fill(vol, axis, lo_map, hi_map, rect, op)
        assert np.array_equal(got, want), (S, axis, op, differing(got, want))
        volume.close()
    src.close()
    dst.close()


@pytest.mark.parametrize("depth", [8, 10])
def test_counters_of_a_full_volume(built, depth):
    """the high planes of the counters: columns of 256 and of 1024 solid voxels.  Records of a small rect and counts of
    boxes; nothing dense is downloaded."""
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    src, dst = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
    src.fillBoxes([[0, 0, 0, S, S, S]])
    src.fillColumns(1, S // 2, S // 2 + 1, (2, 8, 4, 24), model.ANDNOT)            # a notch in the middle of 2 x 16 columns
    rect = (1, 7, 5, 25)
    notched = np.zeros((4, 18), bool)
    notched[1:3, 1:17] = True
    for direction in model.DIRECTIONS:
        axis, side = direction >> 1, direction & 1
        got = src.columnProfile(direction, rect)
        first, last = (0, S - 1) if side else (S - 1, 0)
        if axis == 1:
            want = np.empty(notched.shape, model.COLUMN_DTYPE)
            want[...] = (first, last, S, 1)
            want[notched] = (first, last, S - 1, 2)
            assert np.array_equal(got, want), (depth, direction, record_diff(got, want))
        else:
            assert (got["first"] == first).all() and (got["last"] == last).all() and (got["runs"] == 1).all()
            assert set(np.unique(got["count"]).tolist()) <= {S, S - 1} and (got["count"] == S).any()
    # the voxels with S - 2 or S - 1 solid ones before them, travelling up y: the top layer, and under it only the notched columns
    src.selectColumns(3, S - 2, S + 1, model.SOLID, dst)
    top, under = [0, S - 1, 0, S, S, S], [0, S - 2, 0, S, S - 1, S]
    assert dst.countBoxes([top, under]).tolist() == [S * S, S * S - 32] and dst.solidCount() == 2 * S * S - 32
    src.selectColumns(2, S - 2, S, model.BOTH, dst)                                # travelling down: the same at the bottom
    assert dst.countBoxes([[0, 0, 0, S, 1, S], [0, 1, 0, S, 2, S]]).tolist() == [S * S, S * S - 32] and dst.solidCount() == 2 * S * S - 32
    src.close()
    dst.close()


# ---- 6. the terrain loop --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [6, 8])
def test_heights_to_volume_to_scene(built, depth):
    import cpuvoxelraycaster_amd as vrc
    import oracle_lib as O
    S = 1 << depth
    h = np.ascontiguousarray(O.load_terrain_heights()[:S, :S])
    want = terrain_volume(h, depth)
    volume = vrc.VoxelVolume(depth)
    volume.fillBoxes([[0, 0, 0, S, 3, S]])                                         # raiseTerrain replaces what was there
    assert volume.raiseTerrain(h) is volume
    got = volume.download()
    assert np.array_equal(got, want), differing(got, want)
    assert np.array_equal(want, model.raise_terrain(h, depth))
    scene = vrc.LSVO.fromTerrain(h, depth)
    assert same(committed(volume), scene.downloadNodes())                          # the scene vrc_scene_build_terrain builds
    scene.close()
    lim = np.maximum(16, np.minimum(S, h.astype(np.int64)))
    from_above = 2                                                                 # axis y, towards smaller y: enters at the high-y face
    assert np.array_equal(volume.heightMap(from_above), np.minimum(S // 2 + lim - 1, S - 1).astype(np.int32))
    assert np.array_equal(volume.thicknessMap(1), np.minimum(S // 2 + lim, S) - (S // 2 + 1))
    assert volume.isHeightField(from_above) and not volume.isHeightField(from_above, grounded=True)
    # dig a sphere into the steepest slope, just under the surface of its higher column: the column keeps its top voxel
    top = np.minimum(S // 2 + lim - 1, S - 1)
    step = np.abs(np.diff(top, axis=0))
    x, z = np.unravel_index(np.argmax(step), step.shape)
    tall = x if top[x, z] >= top[x + 1, z] else x + 1
    centre = (int(tall), int(top[tall, z]) - 3, int(z), 2)
    volume.fillSpheres([centre], False)
    dug = want.copy()
    g = np.indices((S, S, S))
    dug[((g[0] - centre[0]) ** 2 + (g[1] - centre[1]) ** 2 + (g[2] - centre[2]) ** 2) <= 4] = 0
    assert dug[tall, top[tall, z], z] and not model.is_height_field(dug, from_above)
    assert not volume.isHeightField(from_above)
    assert volume.columnProfile(from_above, (tall, z, tall + 1, z + 1))[0, 0]["runs"] == 2
    volume.close()
