"""The contacts of posed pieces with a world, on the GPU (vrc_rigid_contacts; VoxelLabels.contacts / contactsDevice / collides).
The expected records are the numpy model's (tests/contact_model.py, held against hand-written cases in
tests/test_volume_contacts_host.py), records written out by hand and closed forms where a test says so, and the library's own
placement where the calls must agree.  Every comparison is exact."""

import numpy as np
import pytest

import components_model
import contact_model as model
import fall_model
import rigid_model
import stamp_model
from volume_support import Stream, affine_records, differing, labels_of, tuples, volume_of

pytestmark = pytest.mark.gpu
IDENTITY = (list(stamp_model.IDENTITY[0]), [0, 0, 0])


# ---- against the model -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [5, 6])
def test_many_pieces_each_under_its_own_pose(built, seed):
    """rigid_model.pose_case at 32^3 -- signed permutations, general rotations, scales, pieces that land on each other,
    clipped, empty and inverted boxes, a map that reads far outside the source, a keep mask -- against three worlds; every
    field of every record.  NULL boxes and NULL keep as well; collides() is overlap > 0."""
    debris, ids, maps, boxes, keep, base = rigid_model.pose_case(32, seed)
    labels = labels_of(debris, 6)
    assert labels.count == len(maps)
    records = affine_records(maps)
    sets = model.posed_sets(ids, maps, boxes, 32, keep)
    for name, world in model.worlds(32, seed):
        star = model.walled(world)
        want = [model.record(A, star) for A in sets]
        assert sum(w[1] > 0 for w in want) > 5 and sum(w[4] > 0 for w in want) > 5, name
        volume = volume_of(world)
        got = tuples(labels.contacts(records, volume, boxes, keep))
        assert got == want, (name, differing(got, want))
        assert labels.collides(records, volume, boxes, keep).tolist() == [w[1] > 0 for w in want]
        volume.close()
    volume = volume_of(base)
    want = model.contacts(ids, maps, None, base)
    got = tuples(labels.contacts(records, volume))
    assert got == want, differing(got, want)
    volume.close()
    labels.close()


@pytest.mark.parametrize("S,connectivity", [(16, 6), (16, 26), (32, 6), (32, 26)])
def test_random_debris_against_worlds_of_32_cubed(built, S, connectivity):
    """rigid_model.random_debris at 16^3 and 32^3 under both connectivities -- boxes, specks, pieces that touch by edges --
    under the maps, boxes and keep mask of rigid_model.pose_case(32, .), taken in turn (the world is 32^3 either way, so it
    differs in depth from the 16^3 labels), and piece 0 at the identity; three worlds, every field of every record"""
    vol = rigid_model.random_debris(S, 40 + S + connectivity)
    ids, rec = components_model.label(vol, connectivity)
    _, _, pose_maps, pose_boxes, pose_keep, _ = rigid_model.pose_case(32, 40 + S + connectivity)
    C_ = len(rec)
    maps = [pose_maps[i % len(pose_maps)] for i in range(C_)]
    boxes = np.array([pose_boxes[i % len(pose_maps)] for i in range(C_)], np.uint32)
    keep = np.array([pose_keep[i % len(pose_maps)] for i in range(C_)], np.uint8)
    maps[0], boxes[0], keep[0] = IDENTITY, [0, 0, 0, 32, 32, 32], 1
    labels = labels_of(vol, connectivity)
    assert labels.count == C_
    records = affine_records(maps)
    sets = model.posed_sets(ids, maps, boxes, 32, keep)
    assert sum(A is not None and A.any() for A in sets) > 8
    for name, world in model.worlds(32, S + connectivity):
        star = model.walled(world)
        want = [model.record(A, star) for A in sets]
        volume = volume_of(world)
        got = tuples(labels.contacts(records, volume, boxes, keep))
        assert got == want, (name, differing(got, want))
        volume.close()
    labels.close()


@pytest.mark.parametrize("axis,sign", model.DIRECTIONS)
def test_every_bit_position_and_face_of_a_word(built, axis, sign):
    """one-voxel pieces moved to each of the 32 bit positions of a word, a one-voxel obstacle on one side: touch 1 with the
    normal from the obstacle to the piece and overlap 0; and the same with the world solid at the piece's voxel too: overlap 1.
    The records are written out by hand in the case and are the model's"""
    ids, targets, maps, boxes, world, expected = model.bit_position_case(axis, sign)
    vol, _, _ = model.specks()
    labels, volume = labels_of(vol), volume_of(world)
    got = tuples(labels.contacts(affine_records(maps), volume, boxes))
    assert got == expected, differing(got, expected)
    got = tuples(labels.contacts(affine_records(maps), volume))              # NULL boxes: every word of the world
    assert got == expected, differing(got, expected)
    volume.close()
    labels.close()


def test_walls_and_a_piece_partly_beyond_the_volume(built):
    """blocks of 27 voxels flat against each of the six faces of an empty world, in its corner, and one layer beyond a face"""
    import cpuvoxelraycaster_amd as vrc
    vol, offsets = model.wall_case()
    ids, rec = components_model.label(vol, 6)
    maps = rigid_model.translation_maps(offsets)
    labels, empty = labels_of(vol), vrc.VoxelVolume(5)
    want = model.contacts(ids, maps, None, np.zeros_like(vol))
    got = labels.contacts(affine_records(maps), empty)
    assert tuples(got) == want, differing(tuples(got), want)
    assert got["touch_n"][:6].tolist() == [[9, 0, 0], [-9, 0, 0], [0, 9, 0], [0, -9, 0], [0, 0, 9], [0, 0, -9]]
    assert (got["posed"][:7] == 27).all() and got["touch"].tolist() == [9] * 6 + [19, 9] and not got["overlap"].any()
    assert got["posed"][7] == 18 < rec["voxels"][7]                          # what leaves the volume is not posed
    assert not labels.collides(affine_records(maps), empty).any()
    empty.close()
    labels.close()


def test_a_world_of_4_cubed(built):
    """a 4^3 world has two occupancy words, shared by its brick rows.  Three pieces of a 16^3 labelling shrunk by 4 (point
    sampling) against an empty, a random, a striped and a full world, with boxes and without"""
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
    stripes = np.zeros((4, 4, 4), np.uint8)
    stripes[:, 1::2, :] = 1
    seen = set()
    for world in (np.zeros((4, 4, 4), np.uint8), (rng.random((4, 4, 4)) < 0.5).astype(np.uint8), stripes, np.ones((4, 4, 4), np.uint8)):
        volume = volume_of(world, 2)
        for bx in (boxes, None):
            want = model.contacts(ids, maps, bx, world)
            got = tuples(labels.contacts(affine_records(maps), volume, bx))
            assert got == want, (bx is None, differing(got, want))
            seen.update(i for i, w in enumerate(want) if w[1] and w[4])
        volume.close()
    assert seen == {0, 1, 2}                                                 # every piece both overlapped and touched somewhere
    labels.close()


def test_more_pieces_than_rows_of_the_grid(built):
    """16384 one-voxel pieces (a 32^3 checkerboard under 6-connectivity): more than the 4096 rows of the launch's grid, so a
    row takes several pieces.  Translations with the moved boxes.  Every record against a restatement for one-voxel pieces in
    whole arrays, and that restatement against the model on every 16th piece"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    board = rigid_model.checkerboard(S)
    ids, rec = components_model.label(board, 6)
    C_ = len(rec)
    assert C_ == 16384
    rng = np.random.default_rng(12)
    offsets = rng.integers(-3, 4, (C_, 3)).astype(np.int32)
    keep = (rng.random(C_) < 0.9).astype(np.uint8)
    world = (rng.random((S, S, S)) < 0.2).astype(np.uint8)
    maps = np.zeros(C_, vrc.capi.AFFINE_DTYPE)
    maps["m"][:] = stamp_model.IDENTITY[0]
    maps["t"][:] = -(offsets.astype(np.int64) << 17)
    boxes = rigid_model.moved_boxes(rec, offsets, S)
    # one voxel at p = lo + offset: posed iff kept and inside the volume
    p = rec["lo"].astype(np.int64) + offsets
    there = (keep != 0) & ((p >= 0) & (p < S)).all(1)
    q = np.clip(p, 0, S - 1) + 1
    star = model.walled(world)
    lower = np.stack([star[tuple((q - model.AXES[a]).T)] for a in range(3)], 1).astype(np.int64)
    upper = np.stack([star[tuple((q + model.AXES[a]).T)] for a in range(3)], 1).astype(np.int64)
    inside = there & (star[tuple(q.T)] != 0)
    touch = there & ~inside & ((lower + upper).sum(1) > 0)
    want = np.zeros(C_, vrc.capi.CONTACT_DTYPE)
    want["posed"], want["overlap"], want["touch"] = there, inside, touch
    want["overlap_s1"], want["touch_s1"] = (2 * p + 1) * inside[:, None], (2 * p + 1) * touch[:, None]
    want["overlap_n"], want["touch_n"] = (lower - upper) * inside[:, None], (lower - upper) * touch[:, None]
    some = list(range(0, C_, 16))
    by_model = [model.record(model.posed(ids, i, (list(maps["m"][i]), list(maps["t"][i])), boxes[i], S) if keep[i] else None, star) for i in some]
    assert tuples(want[some]) == by_model
    labels, volume = labels_of(board, 6), volume_of(world)
    got = labels.contacts(maps, volume, boxes, keep)
    assert got.tobytes() == want.tobytes(), differing(tuples(got), tuples(want))
    assert 1000 < inside.sum() and 1000 < touch.sum() and (~there).sum() > 1000
    volume.close()
    labels.close()


def test_device_memory_on_a_stream_and_a_map_beyond_the_limits(built):
    """keep, maps, boxes and the records in device memory on a created stream: a map beyond the limits, which the host
    cannot see there, gives a zero record and leaves the others as they are; the world's bytes do not change; two calls give
    identical bytes; nothing is written around the records; the labels and the world keep no scratch"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    debris, ids, maps, boxes, keep, base = rigid_model.pose_case(32, 7)
    maps = list(maps)
    keep[[2, 4, 11]] = 1
    legal = affine_records(maps)
    maps[2] = ([(1 << 20) + 1] + list(maps[2][0][1:]), maps[2][1])
    maps[4] = (maps[4][0], [maps[4][1][0], -(1 << 40) - 1, maps[4][1][2]])
    records = affine_records(maps)
    records["reserved"][11] = 1
    labels, world = labels_of(debris, 6), volume_of(base)
    with pytest.raises(vrc.VrcError, match="piece 2: m\\[0\\]"):
        labels.contacts(records, world, boxes, keep)
    all_legal = labels.contacts(legal, world, boxes, keep)
    want = all_legal.copy()
    want[[2, 4, 11]] = np.zeros(1, vrc.capi.CONTACT_DTYPE)[0]
    assert tuples(all_legal) == model.contacts(ids, [(list(r["m"]), list(r["t"])) for r in legal], boxes, base, keep)
    assert all(all_legal["posed"][i] > 0 for i in (2, 4, 11))                # the three would have shown
    before_bytes, before_scratch = labels.bytes(), world.editScratchBytes()
    C_ = labels.count
    t_maps = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    t_boxes = torch.from_numpy(boxes.view(np.int32).copy()).cuda()
    t_keep = torch.from_numpy(keep.copy()).cuda()
    t_out = torch.from_numpy(np.full((C_ + 2) * 128, 0x5A, np.uint8)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        labels.contactsDevice(t_maps.data_ptr(), world, t_out.data_ptr() + 128, t_boxes.data_ptr(), t_keep.data_ptr(), stream)
        vrc.capi.load().vrc_stream_synchronize(0, stream)
        once = t_out.cpu().numpy().copy()
        labels.contactsDevice(t_maps.data_ptr(), world, t_out.data_ptr() + 128, t_boxes.data_ptr(), t_keep.data_ptr(), stream)
    twice = t_out.cpu().numpy()
    assert once.tobytes() == twice.tobytes()
    assert once[128:128 + 128 * C_].tobytes() == want.tobytes()
    assert (once[:128] == 0x5A).all() and (once[128 + 128 * C_:] == 0x5A).all()
    assert np.array_equal(world.download(), base)
    assert labels.bytes() == before_bytes and world.editScratchBytes() == before_scratch
    world.close()
    labels.close()


def test_totals_beyond_32_bits(built):
    """256^3, one full-cube piece at the identity pose over the full world -- the labelled medium itself, from which nothing
    is excluded: every voxel overlaps, every neighbour is solid or a wall, so no normal and no touch; the sum of c is
    S^4 = 2^32 per axis, the smallest cube at which a sum leaves 32 bits.  Closed form"""
    import cpuvoxelraycaster_amd as vrc
    S = 256
    medium = vrc.VoxelVolume(8)
    medium.fillBoxes([[0, 0, 0, S, S, S]])
    labels = medium.labelComponents(6)
    assert labels.count == 1
    n, s1, _ = rigid_model.solid_cube_moments(S)
    assert n == 1 << 24 and s1 == [1 << 32] * 3
    got = tuples(labels.contacts(affine_records([IDENTITY]), medium))
    assert got == [(n, n, s1, [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])]
    # moved by one along x: one layer leaves the volume, and the world being full the rest still only overlaps
    got = tuples(labels.contacts(affine_records(rigid_model.translation_maps([[1, 0, 0]])), medium))
    assert got == [(n - S * S, n - S * S, [s1[0] - S * S, s1[1] - S ** 3, s1[2] - S ** 3], [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])]
    medium.close()
    labels.close()


# ---- against the library's own calls ---------------------------------------------------------------------------------

def test_overlap_is_the_placement_anded_with_the_world(built):
    """placeAffine of piece i alone into an empty volume: its solid count is `posed`, and ANDed with the world and counted with
    countBoxes it is `overlap`"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    debris, ids, maps, boxes, keep, base = rigid_model.pose_case(S, 6)
    labels, world = labels_of(debris, 6), volume_of(base)
    records = affine_records(maps)
    got = labels.contacts(records, world, boxes)
    whole, size = [[0, 0, 0, S, S, S]], (S, S, S)
    shown = 0
    for i in range(0, labels.count, 4):
        only = np.zeros(labels.count, np.uint8)
        only[i] = 1
        placed = labels.placeAffine(records, boxes, None, vrc.capi.VRC_COPY_OR, only)
        assert placed.solidCount() == got["posed"][i], i
        outside = placed.clone()
        outside.copyRegion(world, (0, 0, 0), size, (0, 0, 0), vrc.capi.VRC_COPY_ANDNOT)       # placed and not world
        placed.copyRegion(outside, (0, 0, 0), size, (0, 0, 0), vrc.capi.VRC_COPY_ANDNOT)      # placed and world
        assert int(placed.countBoxes(whole)[0]) == got["overlap"][i], i
        shown += got["overlap"][i] > 0
        placed.close()
        outside.close()
    assert shown > 5
    world.close()
    labels.close()


def test_dig_label_fall_contacts(built):
    """end to end at 32^3: dig, keepConnected, label the debris, fall over the supported part, contacts at the fall's offsets
    against the supported part: the model's records, and no overlap for any piece -- the fall's guarantee on a scene with no
    overlap on entry; every piece rests on something below it"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    vol, supported, debris = model.end_to_end_case(S)
    ids, rec = components_model.label(debris, 6)
    world = volume_of(vol)
    loose = world.keepConnected([[0, 0, 0, S, 1, S]], 6)                      # world keeps the supported part
    assert np.array_equal(world.download(), supported) and np.array_equal(loose.download(), debris)
    labels = loose.labelComponents(6)
    assert labels.count == len(rec) == 2
    offsets, stats = labels.fall(world, vrc.capi.VRC_FACE_YN)
    assert np.array_equal(offsets, fall_model.offsets_of(fall_model.drops(ids, supported, vrc.capi.VRC_FACE_YN), vrc.capi.VRC_FACE_YN))
    maps = rigid_model.translation_maps(offsets)
    boxes = rigid_model.moved_boxes(labels.components(), offsets, S)
    got = labels.contacts(affine_records(maps), world, boxes)
    assert tuples(got) == model.contacts(ids, maps, boxes, supported)
    assert not got["overlap"].any() and (got["posed"] == rec["voxels"]).all()
    assert (got["touch"] > 0).all() and (got["touch_n"][:, 1] > 0).all()
    # one cell further down every piece is inside what it rested on
    deeper = rigid_model.translation_maps(offsets + np.array([0, -1, 0]))
    assert labels.collides(affine_records(deeper), world).all()
    for v in (labels, loose, world):
        v.close()
