"""The pieces of a labelling as rigid bodies with a pose, on the GPU (vrc_rigid_moments, vrc_rigid_place_affine;
VoxelLabels.moments / massProperties / poses / placeAffine).  The expected values are the numpy model's (tests/rigid_model.py,
held against hand-written cases and the fall model in tests/test_volume_rigid_host.py), closed forms where a test says so,
and the library's own vrc_fall_place / vrc_volume_stamp_affine where the calls must agree.  Every comparison is exact."""

import numpy as np
import pytest

import components_model
import fall_model
import rigid_model as model
import stamp_model
from volume_support import Stream, affine_records, labels_of, volume_of

pytestmark = pytest.mark.gpu
NONE = model.NONE


# ---- moments -----------------------------------------------------------------------------------------------------

def check_moments(labels, want, what):
    """every window of the issue against want (the model's list), in host and in device memory with sentinels around the
    window, twice; `voxels` against the records"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    C_ = labels.count
    assert C_ == len(want), (what, C_, len(want))
    got = labels.moments()
    assert [model.moments_tuple(r) for r in got] == want, what
    assert np.array_equal(got["voxels"], labels.components()["voxels"]), what
    for first, capacity in ((0, C_), (1, 2), (C_ - 1, 5), (C_, 3)):
        part = labels.moments(first, capacity)
        assert part.tobytes() == got[first:first + capacity].tobytes(), (what, first, capacity)
        n = len(part)
        raw = np.full((n + 2) * 80, 0x5A, np.uint8)
        t = torch.from_numpy(raw.copy()).cuda()
        torch.cuda.synchronize()
        with Stream() as stream:
            labels.momentsDevice(first, capacity, t.data_ptr() + 80, stream)
            vrc.capi.load().vrc_stream_synchronize(0, stream)
            once = t.cpu().numpy().copy()
            labels.momentsDevice(first, capacity, t.data_ptr() + 80, stream)
        twice = t.cpu().numpy()
        assert once.tobytes() == twice.tobytes(), (what, first, capacity)
        assert once[80:80 + 80 * n].tobytes() == part.tobytes(), (what, first, capacity)
        assert (once[:80] == 0x5A).all() and (once[80 + 80 * n:] == 0x5A).all(), (what, first, capacity)
    assert vrc.capi.load().vrc_rigid_moments(labels._h, 0, 0, None, vrc.capi.VRC_MEM_HOST, None) == 0


@pytest.mark.parametrize("S,connectivity,through_empty", [(S, c, t) for S in (16, 32) for c in (6, 26) for t in (False, True)])
def test_moments_of_random_debris(built, S, connectivity, through_empty):
    vol = model.random_debris(S, 40 + S + connectivity)
    ids, rec = components_model.label(vol, connectivity, through_empty)
    want = model.moments(ids, len(rec)) if S == 16 else model.moments_fast(ids, len(rec))
    labels = labels_of(vol, connectivity, through_empty)
    before = labels.bytes()
    check_moments(labels, want, (S, connectivity, through_empty))
    assert labels.bytes() == before                     # stateless: the snapshot gained nothing
    labels.close()


def test_moments_uniform_waves_one_id_per_lane_and_two_ids_per_word(built):
    """the three aggregation paths: a full 32^3 solid (every wave uniform; closed form), a 16^3 checkerboard under
    6-connectivity (2048 one-voxel pieces: every lane its own id), two interlocking combs (two ids in every word)"""
    S = 32
    labels = labels_of(np.ones((S, S, S), np.uint8))
    n, s1, s2 = model.solid_cube_moments(S)
    assert s1 == [n * S] * 3
    check_moments(labels, [(n, s1, s2)], "solid")
    labels.close()
    board = model.checkerboard(16)
    ids, rec = components_model.label(board, 6)
    assert len(rec) == 2048
    labels = labels_of(board, 6)
    check_moments(labels, model.moments(ids, 2048), "checkerboard")
    labels.close()
    for S in (16, 32):
        combs = model.combs(S)
        ids, rec = components_model.label(combs, 6)
        assert len(rec) == 2
        labels = labels_of(combs, 6)
        check_moments(labels, model.moments_fast(ids, 2), ("combs", S))
        labels.close()


def test_moments_accumulate_in_64_bits(built):
    """a full 128^3 solid: the smallest cube whose sum of c_x^2 (4.58e10) exceeds 2^32; closed form"""
    import cpuvoxelraycaster_amd as vrc
    S = 128
    medium = vrc.VoxelVolume(7)
    medium.fillBoxes([[0, 0, 0, S, S, S]])
    labels = medium.labelComponents(6)
    medium.close()
    want = model.solid_cube_moments(S)
    assert want[2][0] > 1 << 32
    got = labels.moments()
    assert labels.count == 1 and model.moments_tuple(got[0]) == want
    assert got["voxels"][0] == labels.components()["voxels"][0] == S ** 3
    mass, centre, inertia = labels.massProperties()
    assert mass[0] == S ** 3 and centre[0].tolist() == [64.0] * 3
    assert inertia[0].tolist() == [[float(S ** 3) * S * S / 6 if a == b else 0.0 for b in range(3)] for a in range(3)]
    labels.close()


# ---- placement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,connectivity,direction,limit,seed", fall_model.RANDOM_CASES[::4])
def test_translation_maps_are_the_fall_place(built, S, connectivity, direction, limit, seed):
    """pure translations: the device's vrc_fall_place with the same offsets, and the model; with the moved record boxes and
    with NULL boxes, OR into a random base and ANDNOT out of it"""
    import cpuvoxelraycaster_amd as vrc
    debris, fixed = fall_model.random_case(S, seed)
    ids, rec = components_model.label(debris, connectivity)
    rng = np.random.default_rng(seed)
    offsets = rng.integers(-S // 3, S // 3 + 1, (len(rec), 3)).astype(np.int32)
    offsets[::5] = fall_model.offsets_of(np.full(len(rec), 3)[::5], direction)
    keep = (rng.random(len(rec)) < 0.8).astype(np.uint8)
    maps = affine_records(model.translation_maps(offsets))
    labels = labels_of(debris, connectivity)
    records = labels.components()
    boxes = model.moved_boxes(records, offsets, S)
    for op, op_or in ((vrc.capi.VRC_COPY_OR, True), (vrc.capi.VRC_COPY_ANDNOT, False)):
        want = fall_model.place(ids, offsets, fixed, op_or, keep)
        by_fall = volume_of(fixed)
        labels.place(offsets, by_fall, op, keep)
        assert np.array_equal(by_fall.download(), want)
        by_fall.close()
        for bx in (boxes, None):
            dst = volume_of(fixed)
            assert labels.placeAffine(maps, bx, dst, op, keep) is dst
            assert np.array_equal(dst.download(), want), (op, bx is None)
            dst.close()
    labels.close()


def one_piece_cases(S):
    r = stamp_model.rotation
    half = S / 2
    quarter = stamp_model.signed_permutation((1, 0, 2), (0, 1, 0), S)
    thirty = stamp_model.place(stamp_model.compose(r(0, np.pi / 6), r(1, np.pi / 6)), 1.0, (half,) * 3, (half,) * 3, 5, 5)
    double = stamp_model.place(r(2, 0.4), 2.0, (half,) * 3, (half,) * 3, 5, 5)
    halved = stamp_model.place(r(1, -0.7), 0.5, (half,) * 3, (half,) * 3, 5, 5)
    return [("quarter", quarter[0], quarter[1], (0, 0, 0), (S, S, S)), ("thirty", thirty[0], thirty[1], (3, 0, 5), (S - 2, S, S - 7)),
            ("double", double[0], double[1], (0, 0, 0), (S, S, S)), ("halved", halved[0], halved[1], (1, 1, 1), (S - 1, S - 1, S - 1))]


def test_one_piece_is_the_stamp_of_the_selected_volume(built):
    """C = 1: vrc_volume_stamp_affine of the piece's own volume with the same map and box -- a quarter turn (the voxel count
    is preserved), a 30-degree turn about two axes, scale 2, scale 1/2 -- and the 30-degree turn into a 64^3 destination"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    rng = np.random.default_rng(3)
    piece = np.zeros((S, S, S), np.uint8)
    piece[6:25, 9:21, 4:27] = 1
    piece[8:12, 9:21, 10:20] = 0
    piece[24:29, 12:15, 12:15] = 1
    ids, rec = components_model.label(piece, 6)
    assert len(rec) == 1
    labels = labels_of(piece, 6)
    source = labels.select([1])
    assert np.array_equal(source.download(), piece)
    base = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
    for name, m, t, lo, hi in one_piece_cases(S):
        a = vrc.make_affine(m, t)
        for op in (vrc.capi.VRC_COPY_OR, vrc.capi.VRC_COPY_ANDNOT):
            by_stamp, dst = volume_of(base), volume_of(base)
            by_stamp.stampAffine(source, a, lo, hi, op)
            labels.placeAffine([a], [list(lo) + list(hi)], dst, op)
            got = dst.download()
            assert np.array_equal(got, by_stamp.download()), (name, op)
            assert np.array_equal(got, model.place_affine(ids, [(m, t)], [list(lo) + list(hi)], base, op)), (name, op)
            if name == "quarter" and op == vrc.capi.VRC_COPY_OR:
                clean = labels.placeAffine([a])
                assert clean.solidCount() == int(piece.sum())
                clean.close()
            by_stamp.close()
            dst.close()
    # into a destination of another depth: 32^3 labels turned and doubled into 64^3
    m, t, lo, hi = stamp_model.place(stamp_model.compose(stamp_model.rotation(0, np.pi / 6), stamp_model.rotation(1, np.pi / 6)), 2.0, (16,) * 3, (30, 34, 31), 5, 6)
    a = vrc.make_affine(m, t)
    by_stamp, dst = vrc.VoxelVolume(6), vrc.VoxelVolume(6)
    by_stamp.stampAffine(source, a, lo, hi, vrc.capi.VRC_COPY_OR)
    labels.placeAffine([a], [list(lo) + list(hi)], dst)
    got = dst.download()
    assert got.any() and np.array_equal(got, by_stamp.download())
    assert np.array_equal(got, model.place_affine(ids, [(m, t)], [list(lo) + list(hi)], np.zeros((64, 64, 64), np.uint8)))
    for v in (by_stamp, dst, source, labels):
        v.close()


@pytest.mark.parametrize("seed", [5, 6])
def test_many_pieces_each_through_its_own_map(built, seed):
    """32^3, pieces that touch by corners, seeded signed permutations and general rotations, pieces that land on each other,
    a keep mask with zeros, boxes with odd corners and clipped, empty and inverted ones, a map that reads outside the
    source; base is random bits and every voxel of dst is compared"""
    import cpuvoxelraycaster_amd as vrc
    debris, ids, maps, boxes, keep, base = model.pose_case(32, seed)
    labels = labels_of(debris, 6)
    assert labels.count == len(maps)
    records = affine_records(maps)
    for op, model_op in ((vrc.capi.VRC_COPY_OR, model.OR), (vrc.capi.VRC_COPY_ANDNOT, model.ANDNOT)):
        want = model.place_affine(ids, maps, boxes, base, model_op, keep)
        assert not np.array_equal(want, base)
        dst = volume_of(base)
        labels.placeAffine(records, boxes, dst, op, keep)
        once = dst.download()
        assert np.array_equal(once, want), op
        again = volume_of(base)
        labels.placeAffine(records, boxes, again, op, keep)
        assert np.array_equal(again.download(), once)
        dst.close()
        again.close()
    # NULL boxes and NULL keep: every piece over all of dst
    want = model.place_affine(ids, maps, None, base, model.OR, None)
    dst = volume_of(base)
    labels.placeAffine(records, None, dst)
    assert np.array_equal(dst.download(), want)
    dst.close()
    labels.close()


def test_into_a_destination_of_4_cubed(built):
    """a 4^3 destination has two occupancy words, shared by its brick rows: the lanes of a wave that hit one word join their
    bits.  Three pieces of a 16^3 labelling shrunk by 4 (point sampling), overlapping in dst, against the model"""
    import cpuvoxelraycaster_amd as vrc
    S = 16
    debris = np.zeros((S, S, S), np.uint8)
    debris[0:9, 0:16, 0:7] = 1
    debris[10:16, 2:14, 0:16] = 1
    debris[0:8, 3:9, 9:16] = 1
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 3
    quarter = [4 * stamp_model.ONE if a == b else 0 for a in range(3) for b in range(3)]
    turned = [0, 4 * stamp_model.ONE, 0, -4 * stamp_model.ONE, 0, 0, 0, 0, 4 * stamp_model.ONE]
    maps = [(quarter, [0, 0, 0]), (quarter, [-(3 << 17), 1 << 16, 0]), (turned, [0, 16 << 17, 5 << 15])]
    boxes = np.array([[0, 0, 0, 4, 4, 4], [1, 0, 0, 4, 3, 4], [0, 0, 1, 4, 4, 0xFFFFFFFF]], np.uint32)
    labels = labels_of(debris, 6)
    rng = np.random.default_rng(9)
    for base in (np.zeros((4, 4, 4), np.uint8), (rng.random((4, 4, 4)) < 0.5).astype(np.uint8)):
        for op, model_op in ((vrc.capi.VRC_COPY_OR, model.OR), (vrc.capi.VRC_COPY_ANDNOT, model.ANDNOT)):
            for bx in (boxes, None):
                want = model.place_affine(ids, maps, bx, base if model_op == model.OR else 1 - base, model_op)
                dst = volume_of(base if model_op == model.OR else 1 - base, 2)
                labels.placeAffine(affine_records(maps), bx, dst, op)
                assert np.array_equal(dst.download(), want), (op, bx is None)
                dst.close()
    each = [model.place_affine(ids, [mp if j == i else (mp[0], [1 << 50] * 3) for j, mp in enumerate(maps)], None, np.zeros((4, 4, 4), np.uint8)) for i in range(3)]
    assert all(e.any() for e in each) and (np.sum(each, axis=0) > 1).any()          # every piece shows, and two share a voxel
    labels.close()


def test_more_pieces_than_rows_of_the_grid(built):
    """16384 one-voxel pieces (a 32^3 checkerboard under 6-connectivity): more than the 4096 rows of the launch's grid, so
    a row takes several pieces.  Translations, against the fall model's scatter; with boxes and with NULL boxes"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    board = model.checkerboard(S)
    ids, rec = components_model.label(board, 6)
    assert len(rec) == 16384
    rng = np.random.default_rng(12)
    offsets = rng.integers(-3, 4, (len(rec), 3)).astype(np.int32)
    keep = (rng.random(len(rec)) < 0.9).astype(np.uint8)
    base = (rng.random((S, S, S)) < 0.2).astype(np.uint8)
    maps = np.zeros(len(rec), vrc.capi.AFFINE_DTYPE)
    maps["m"][:] = stamp_model.IDENTITY[0]
    maps["t"][:] = -(offsets.astype(np.int64) << 17)
    labels = labels_of(board, 6)
    boxes = model.moved_boxes(labels.components(), offsets, S)
    want = fall_model.place(ids, offsets, base, True, keep)
    for bx in (boxes, None):
        dst = volume_of(base)
        labels.placeAffine(maps, bx, dst, vrc.capi.VRC_COPY_OR, keep)
        assert np.array_equal(dst.download(), want), bx is None
        dst.close()
    labels.close()


def test_device_memory_on_a_stream_and_a_map_beyond_the_limits(built):
    """maps, boxes and keep in device memory on a created stream, then download (ordered behind it: it is dst's last edit); a
    map beyond the limits, which the host cannot see there, drops that piece alone"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    debris, ids, maps, boxes, keep, base = model.pose_case(32, 7)
    maps = list(maps)
    maps[2] = ([(1 << 20) + 1] + list(maps[2][0][1:]), maps[2][1])
    maps[4] = (maps[4][0], [maps[4][1][0], -(1 << 40) - 1, maps[4][1][2]])
    keep[[2, 4, 11]] = 1
    records = affine_records(maps)
    records["reserved"][11] = 1
    labels = labels_of(debris, 6)
    with pytest.raises(vrc.VrcError, match="piece 2: m\\[0\\]"):
        labels.placeAffine(records, boxes, None, vrc.capi.VRC_COPY_OR, keep)
    dropped = list(maps)
    dropped[11] = (maps[11][0], [1 << 50] * 3)
    want = model.place_affine(ids, dropped, boxes, base, model.OR, keep)
    legal = list(dropped)
    for i in (2, 4, 11):
        legal[i] = (list(stamp_model.IDENTITY[0]), [0, 0, 0])
    assert not np.array_equal(want, model.place_affine(ids, legal, boxes, base, model.OR, keep))      # the three would have shown
    t_maps = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    t_boxes = torch.from_numpy(boxes.view(np.int32).copy()).cuda()
    t_keep = torch.from_numpy(keep.copy()).cuda()
    torch.cuda.synchronize()
    dst = volume_of(base)
    with Stream() as stream:
        labels.placeAffineDevice(t_maps.data_ptr(), dst, t_boxes.data_ptr(), vrc.capi.VRC_COPY_OR, t_keep.data_ptr(), stream)
        got = dst.download()
    assert np.array_equal(got, want)
    dst.close()
    labels.close()


def test_dig_label_pose_place_commit(built):
    """end to end at 32^3: dig, keepConnected, label the debris, mass properties, poses about the centres of mass,
    placeAffine into the world, commit: the committed scene's nodes are the host builder's on the model's volume"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[:, 0:3, :] = 1
    vol[14:18, 3:28, 14:18] = 1
    x, y, z = np.indices((S, S, S))
    vol[(x - 16) ** 2 + (y - 12) ** 2 + (z - 16) ** 2 <= 25] = 0
    vol[4:9, 20:23, 5:12] = 1
    whole, _ = components_model.label(vol, 6)
    supported = (whole == whole[0, 0, 0]).astype(np.uint8)
    debris = vol & (1 - supported)
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 2

    world = volume_of(vol)
    loose = world.keepConnected([[0, 0, 0, S, 1, S]], 6)
    labels = loose.labelComponents(6)
    assert labels.count == 2
    mass, centre, inertia = labels.massProperties()
    for i, case in enumerate(model.moments(ids, 2)):
        m, c, I = model.mass_properties(*case)
        assert mass[i] == float(m) and centre[i].tolist() == [float(v) for v in c]
        assert inertia[i].tolist() == [[float(v) for v in row] for row in I]
    rot = stamp_model.compose(stamp_model.rotation(0, np.pi / 6), stamp_model.rotation(2, np.pi / 6))
    target = centre + np.array([[3.0, -4.0, 2.0], [-1.0, -9.0, 5.0]])
    maps, boxes = labels.poses(rot, target)
    expect = [model.place_box(rot, 1.0, centre[i], target[i], rec["lo"][i], rec["hi"][i], 5) for i in range(2)]
    assert [(list(r["m"]), list(r["t"])) for r in maps] == [(m, t) for m, t, _, _ in expect]
    assert boxes.tolist() == [lo + hi for _, _, lo, hi in expect]
    labels.placeAffine(maps, boxes, world)
    want = model.place_affine(ids, [(m, t) for m, t, _, _ in expect], boxes, supported)
    assert int(want.sum()) > int(supported.sum())
    assert np.array_equal(world.download(), want)
    svo = world.commit()
    assert svo.downloadNodes().tobytes() == vrc.build_volume_lsvo(want, 5).tobytes()
    for v in (svo, labels, loose, world):
        v.close()
