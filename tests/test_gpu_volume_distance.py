"""The exact squared Euclidean distance field on the GPU (vrc_volume_distance_field, vrc_distance_*;
VoxelVolume.distanceField / VoxelDistance, dilate / erode / openShape / closeShape / hollow).  The expected field is the
numpy model of tests/distance_model.py (held against the definition in tests/test_volume_distance_host.py), or the analytic
answer where a test says so.  Every comparison is exact."""

import numpy as np
import pytest

import distance_model as model
from volume_support import Stream, all_coordinates, volume_of

pytestmark = pytest.mark.gpu

NONE = model.NONE


def check_stats(field, D, features, what):
    m, arg = model.stats(D)
    s = field.stats
    assert (int(s.features), int(s.max_d2), tuple(int(v) for v in s.argmax), int(s.reserved)) == (features, m, arg, 0), what


def check_field(field, D, features, what, with_at=True):
    """download(), at() of everything, stats and bytes() against an expected field"""
    S = D.shape[0]
    got = field.download()
    assert got.dtype == np.uint32 and got.shape == (S, S, S)
    assert np.array_equal(got, D), (what, int((got != D).sum()))
    if with_at:
        at = field.at(all_coordinates(S))
        assert np.array_equal(at[:S ** 3].reshape(S, S, S), D), what
        assert (at[S ** 3:] == NONE).all(), what
    check_stats(field, D, features, what)
    assert field.bytes() == 4 * S ** 3 and field.depth == S.bit_length() - 1 and field.data_ptr() != 0


# ---- random volumes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_random_volumes(built, depth):
    """Depth 2 is a single occupancy word per brick-row pair, 5 one 32-voxel tile, 6 one full wave along z; densities from
    almost empty (long parabolas) to almost full, both feature sets, faces as walls and open."""
    S = 1 << depth
    rng = np.random.default_rng(9000 + depth)
    for density in (0.002, 0.05, 0.5, 0.95):
        vol = (rng.random((S, S, S)) < density).astype(np.uint8)
        volume = volume_of(vol, depth)
        for to_empty in (False, True):
            features = int(model.feature_set(vol, to_empty).sum())
            inside = model.field(vol, to_empty, False)
            for outside in (False, True):
                D = model.open_border(inside) if outside else inside
                field = volume.distanceField(to_empty, outside)
                check_field(field, D, features, (depth, density, to_empty, outside))
                field.close()
        volume.close()


# ---- constructed cases ------------------------------------------------------------------------------------------

def analytic(S, points):
    c = np.arange(S, dtype=np.int64)
    D = None
    for a, b, cc in points:
        d = ((c - a) ** 2)[:, None, None] + ((c - b) ** 2)[None, :, None] + ((c - cc) ** 2)[None, None, :]
        D = d if D is None else np.minimum(D, d)
    return D.astype(np.uint32)


@pytest.mark.parametrize("where", [(0, 0, 0), (127, 0, 0), (0, 127, 0), (0, 0, 127), (127, 127, 0), (127, 0, 127), (0, 127, 127),
                                   (127, 127, 127), (63, 64, 65)])
def test_one_feature_voxel_at_depth_7(built, where):
    """A line spans two waves; one parabola covers every line, the longest the depth has."""
    depth, S = 7, 128
    vol = np.zeros((S, S, S), np.uint8)
    vol[where] = 1
    D = analytic(S, [where])
    volume = volume_of(vol, depth)
    field = volume.distanceField()
    check_field(field, D, 1, where, with_at=False)
    far = tuple(0 if w >= 64 else S - 1 for w in where)
    assert int(field.stats.max_d2) == sum((f - w) ** 2 for f, w in zip(far, where))
    assert tuple(field.stats.argmax) == far
    if where != (63, 64, 65):
        assert int(field.stats.max_d2) == 3 * 127 ** 2
    probes = np.array([where, far, (64, 64, 64), (S, 0, 0)], np.uint32)
    assert list(field.at(probes)) == [0, int(D[far]), int(D[64, 64, 64]), NONE]
    field.close()
    volume.close()


def test_depth_8_stacks_in_device_scratch(built):
    """From 256^3 on the envelope stacks live in a device block sized by the lines in flight and the z pass takes several
    columns of 8 words per step: a handful of voxels (corners, a word border, a wave border) against the analytic field,
    with the faces as walls and open."""
    depth, S = 8, 256
    points = [(0, 0, 0), (255, 255, 255), (31, 32, 33), (200, 63, 64), (128, 255, 0), (7, 140, 255)]
    vol = np.zeros((S, S, S), np.uint8)
    for p in points:
        vol[p] = 1
    D = analytic(S, points)
    volume = volume_of(vol, depth)
    for outside in (False, True):
        field = volume.distanceField(False, outside)
        check_field(field, model.open_border(D) if outside else D, len(points), ("depth 8", outside), with_at=False)
        field.close()
    # the complement: every voxel but six is a feature
    field = volume.distanceField(True)
    want = np.ones((S, S, S), np.uint32)
    want[vol == 0] = 0
    check_field(field, want, S ** 3 - len(points), "depth 8, to empty", with_at=False)
    field.close()
    volume.close()


@pytest.mark.parametrize("pair", ["x", "y", "z", "diagonal"])
def test_two_voxels_far_apart_at_depth_7(built, pair):
    """Two voxels S - 1 apart along one axis: the envelope's crossover lies on the wave border 63 | 64 (both are equally
    far from 63.5); and at two opposite corners."""
    depth, S = 7, 128
    if pair == "diagonal":
        points = [(0, 0, 0), (127, 127, 127)]
    else:
        axis = "xyz".index(pair)
        p, q = [5, 70, 33], [5, 70, 33]
        p[axis], q[axis] = 0, S - 1
        points = [tuple(p), tuple(q)]
    vol = np.zeros((S, S, S), np.uint8)
    for p in points:
        vol[p] = 1
    volume = volume_of(vol, depth)
    field = volume.distanceField()
    check_field(field, analytic(S, points), 2, pair, with_at=False)
    field.close()
    volume.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_solid_plane_at_depth_6(built, axis):
    """The plane p_axis = 0: D = p_axis^2 everywhere -- equal parabolas, ties along the other two axes, the largest values
    of the depth."""
    depth, S = 6, 64
    vol = np.zeros((S, S, S), np.uint8)
    index = [slice(None)] * 3
    index[axis] = 0
    vol[tuple(index)] = 1
    shape = [1, 1, 1]
    shape[axis] = S
    D = np.broadcast_to((np.arange(S, dtype=np.uint32) ** 2).reshape(shape), (S, S, S))
    assert np.array_equal(D, model.field(vol))
    volume = volume_of(vol, depth)
    field = volume.distanceField()
    check_field(field, D, S * S, axis)
    far = [0, 0, 0]
    far[axis] = S - 1
    assert int(field.stats.max_d2) == (S - 1) ** 2 and tuple(field.stats.argmax) == tuple(far)
    field.close()
    volume.close()


@pytest.mark.parametrize("depth", [2, 5, 6])
def test_empty_and_full(built, depth):
    """outside == 0: all NONE for an empty F (stats 0), all 0 for a full F; outside != 0 with an empty F: the wall term."""
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    empty = vrc.VoxelVolume(depth)
    full = vrc.VoxelVolume(depth)
    full.fillBoxes([[0, 0, 0, S, S, S]])
    wall = model.wall_term(S).astype(np.uint32)
    for volume, to_empty, f_is_empty in [(empty, False, True), (empty, True, False), (full, False, False), (full, True, True)]:
        for outside in (False, True):
            field = volume.distanceField(to_empty, outside)
            if not f_is_empty:
                D = np.zeros((S, S, S), np.uint32)
            elif outside:
                D = wall
            else:
                D = np.full((S, S, S), NONE, np.uint32)
            check_field(field, D, 0 if f_is_empty else S ** 3, (depth, to_empty, f_is_empty, outside))
            if f_is_empty and not outside:
                assert int(field.stats.max_d2) == 0 and tuple(field.stats.argmax) == (0, 0, 0)
            if f_is_empty and outside:
                assert int(field.stats.max_d2) == (S // 2) ** 2 and tuple(field.stats.argmax) == (S // 2 - 1,) * 3
            field.close()
    empty.close()
    full.close()


# ---- the tools, against code that already ships ---------------------------------------------------------------------

def forty_voxels(S, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(0, S, (40, 3))
    xyz[:6] = [[0, 5, 9], [S - 1, 20, 3], [7, 0, 30], [12, S - 1, 1], [3, 4, 0], [S - 1, S - 1, S - 1]]     # on the faces
    return xyz


@pytest.mark.parametrize("r", [0, 1, 2, 3, 5])
def test_dilate_equals_spheres_at_every_voxel(built, r):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 5, 32
    xyz = forty_voxels(S, 77)
    grown = vrc.VoxelVolume(depth)
    grown.setVoxels(xyz)
    assert grown.dilate(r) is grown
    brushed = vrc.VoxelVolume(depth)
    brushed.fillSpheres(np.concatenate([xyz, np.full((len(xyz), 1), r)], axis=1))
    got, want = grown.download(), brushed.download()
    assert np.array_equal(got, want)
    vol = np.zeros((S, S, S), np.uint8)
    vol[tuple(xyz.T)] = 1
    assert np.array_equal(got != 0, model.dilate(vol, r))
    grown.close()
    brushed.close()


@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_erode_is_the_dual_of_dilate(built, r):
    """erode(r) of V with the faces as walls = the complement of dilate(r) of the complement of V; with the border open =
    eroding V embedded in a volume one depth larger with an empty margin, cropped back."""
    import cpuvoxelraycaster_amd as vrc
    depth, S = 5, 32
    rng = np.random.default_rng(500 + r)
    vol = np.zeros((S, S, S), np.uint8)
    vol[0:14, 3:20, 0:S] = 1                                  # touches three faces
    vol[18:S, 10:S, 6:25] = 1
    vol[rng.random((S, S, S)) < 0.01] ^= 1
    eroded = volume_of(vol, depth)
    eroded.erode(r)
    got = eroded.download() != 0
    complement = volume_of(1 - vol, depth)
    complement.dilate(r)
    assert np.array_equal(got, complement.download() == 0)
    assert np.array_equal(got, model.erode(vol, r))
    # open border
    opened = volume_of(vol, depth)
    opened.erode(r, open_border=True)
    big = np.zeros((2 * S, 2 * S, 2 * S), np.uint8)
    big[8:8 + S, 8:8 + S, 8:8 + S] = vol
    embedded = volume_of(big, depth + 1)
    embedded.erode(r)
    want = embedded.download()[8:8 + S, 8:8 + S, 8:8 + S] != 0
    assert np.array_equal(opened.download() != 0, want)
    assert np.array_equal(want, model.erode(vol, r, True))
    for v in (eroded, complement, opened, embedded):
        v.close()


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_hollow_a_box(built, t):
    depth, S = 5, 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[5:25, 6:26, 7:27] = 1
    volume = volume_of(vol, depth)
    volume.hollow(t)
    got = volume.download() != 0
    assert np.array_equal(got, model.hollow(vol, t))
    core = max(20 - 2 * t, 0) if t else 20
    assert int(got.sum()) == 20 ** 3 - core ** 3
    volume.close()


def test_open_and_close_shape(built):
    depth, S = 5, 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[3:9, 3:9, 3:9] = 1                                    # a 6^3 box
    vol[20, 20, 20] = 1                                       # a speck
    vol[12:30, 14, 2:30] = 1                                  # a sheet one voxel thick
    volume = volume_of(vol, depth)
    volume.openShape(1)
    got = volume.download() != 0
    want = model.dilate(model.erode(vol, 1).astype(np.uint8), 1)
    assert np.array_equal(got, want)
    assert not got[20, 20, 20] and not got[12:30, 14, 2:30].any() and got[4:8, 4:8, 4:8].all() and int(got.sum()) == want.sum() > 64
    volume.close()

    holed = np.zeros((S, S, S), np.uint8)
    holed[8:20, 8:20, 8:20] = 1
    holed[13, 14, 15] = 0                                     # a one-voxel hole
    volume = volume_of(holed, depth)
    volume.closeShape(2)
    got = volume.download() != 0
    assert np.array_equal(got, model.erode(model.dilate(holed, 2).astype(np.uint8), 2))
    assert got[13, 14, 15] and got[8:20, 8:20, 8:20].all()
    volume.close()


# ---- select -----------------------------------------------------------------------------------------------------------

def test_select_ops_shells_and_ordering(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    REPLACE, OR, ANDNOT = vrc.capi.VRC_COPY_REPLACE, vrc.capi.VRC_COPY_OR, vrc.capi.VRC_COPY_ANDNOT
    depth, S = 5, 32
    rng = np.random.default_rng(31)
    vol = (rng.random((S, S, S)) < 0.003).astype(np.uint8)
    other = (rng.random((S, S, S)) < 0.4).astype(np.uint8)
    D = model.field(vol)
    medium = volume_of(vol, depth)
    field = medium.distanceField()
    for lo, hi in [(0, 0), (9, 9), (5, 5), (2, 17), (0, NONE), (NONE, NONE), (int(D.max()), NONE)]:
        K = model.select(D, lo, hi)
        fresh = field.select(lo, hi)
        assert np.array_equal(fresh.download(), K), (lo, hi)
        fresh.close()
        for op, want in [(REPLACE, K), (OR, other | K), (ANDNOT, other & (1 - K))]:
            dst = volume_of(other, depth)
            assert field.select(lo, hi, dst, op) is dst
            assert np.array_equal(dst.download(), want), (lo, hi, op)
            dst.close()
    assert int(model.select(D, 9, 9).sum()) > 0 and int(model.select(D, 0, NONE).sum()) == S ** 3
    # dst = the medium itself; the snapshot does not follow
    field.select(1, 4, medium, OR)
    assert np.array_equal(medium.download(), vol | model.select(D, 1, 4))
    assert np.array_equal(field.download(), D)
    # on a created stream right after a device-memory edit of dst on the same stream: the result contains the edit
    dst = volume_of(other, depth)
    extra = np.argwhere(model.select(D, 30, NONE))[:50].astype(np.uint32)
    assert len(extra) == 50
    d_extra = torch.from_numpy(extra.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        dst.setVoxelsDevice(len(extra), d_extra.data_ptr(), True, stream)
        field.select(0, 8, dst, ANDNOT, stream)
    want = other.copy()
    want[tuple(extra.T.astype(np.int64))] = 1
    want &= 1 - model.select(D, 0, 8)
    assert np.array_equal(dst.download(), want)
    # depth 2: two brick rows to a word
    small = np.zeros((4, 4, 4), np.uint8)
    small[1, 2, 3] = 1
    tiny = volume_of(small, 2)
    f2 = tiny.distanceField()
    ring = f2.select(1, 2)
    assert np.array_equal(ring.download(), model.select(model.field(small), 1, 2))
    for v in (ring, f2, tiny, dst, field, medium):
        v.close()


def test_field_as_a_tensor_in_place(built):
    """data_ptr() is an (S, S, S) uint32 field a device-memory caller reads in place: atDevice gathers from it."""
    import torch
    depth, S = 4, 16
    rng = np.random.default_rng(5)
    vol = (rng.random((S, S, S)) < 0.02).astype(np.uint8)
    volume = volume_of(vol, depth)
    field = volume.distanceField(outside=True)
    D = model.field(vol, False, True)
    xyz = all_coordinates(S)
    d_xyz = torch.from_numpy(xyz.view(np.int32).copy()).cuda()
    d_out = torch.zeros(len(xyz), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    field.atDevice(len(xyz), d_xyz.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:S ** 3].reshape(S, S, S), D) and (got[S ** 3:] == NONE).all()
    field.close()
    volume.close()


# ---- snapshot ---------------------------------------------------------------------------------------------------------

def test_snapshot_outlives_edits_and_the_medium(built):
    depth, S = 5, 32
    rng = np.random.default_rng(11)
    vol = (rng.random((S, S, S)) < 0.01).astype(np.uint8)
    volume = volume_of(vol, depth)
    first = volume.distanceField()
    twin = volume.distanceField()
    D = model.field(vol)
    assert first.download().tobytes() == twin.download().tobytes() == D.tobytes()
    edited = vol.copy()
    edited[10:14, 10:14, 10:14] = 1
    edited[tuple(np.argwhere(vol)[0])] = 0
    volume.fillBoxes([[10, 10, 10, 14, 14, 14]])
    volume.setVoxels([np.argwhere(vol)[0]], False)
    second = volume.distanceField()
    volume.close()
    assert np.array_equal(first.download(), D)
    D2 = model.field(edited)
    assert np.array_equal(second.download(), D2) and not np.array_equal(D, D2)
    check_stats(second, D2, int(edited.sum()), "edited")
    for f in (first, twin, second):
        f.close()
