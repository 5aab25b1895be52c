"""A field read at the voxels of posed pieces, on the GPU (vrc_rigid_clearance; VoxelLabels.clearance / clearanceDevice /
freeRadius).  The expected records are the numpy model's (tests/clearance_model.py, held against hand-written cases in
tests/test_volume_clearance_host.py) over the numpy fields of distance_model / travel_model, closed forms where a test says so,
and the library's own vrc_rigid_contacts where the two calls must agree.  Every comparison is exact."""

import numpy as np
import pytest

import clearance_model as model
import components_model
import contact_model
import distance_model
import posed_cases
import rigid_model
import stamp_model
from volume_support import Stream, affine_records, differing, labels_of, volume_of

pytestmark = pytest.mark.gpu
NONE = model.NONE
IDENTITY = (list(stamp_model.IDENTITY[0]), [0, 0, 0])


def field_of(world, spec, depth=None):
    """the device's field of a world: spec = (to_empty, outside) for the Euclidean one, None for the travel field through the
    air from clearance_model.air_seed"""
    volume = volume_of(world, depth)
    if spec is None:
        seeds = volume_of(model.air_seed(world), depth)
        field = volume.travelField(seeds, 6, True)
        seeds.close()
    else:
        field = volume.distanceField(*spec)
    volume.close()
    return field


# ---- against the model -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [5, 6])
def test_many_pieces_each_under_its_own_pose(built, seed):
    """rigid_model.pose_case at 32^3 -- signed permutations, general rotations, scales, pieces that land on each other,
    clipped, empty and inverted boxes, a map that reads far outside the source, a keep mask -- over four fields of its base
    world: the distance to the solid with walls and with an open border, the distance to the empty (penetration depth) and a
    travel field through the air, which holds NONE; every field of every record.  NULL boxes and NULL keep as well."""
    debris, ids, maps, boxes, keep, base = rigid_model.pose_case(32, seed)
    labels = labels_of(debris, 6)
    assert labels.count == len(maps)
    records = affine_records(maps)
    sets = posed_cases.posed_point_sets(ids, maps, boxes, 32, keep)
    whole = posed_cases.posed_point_sets(ids, maps, None, 32)
    for name, spec, D in model.fields_of(base):
        field = field_of(base, spec)
        assert np.array_equal(field.download(), D), name
        want = model.records_of(sets, D)
        assert sum(w[3] != NONE for w in want) > 5, name
        if spec is None:
            assert any(w[1] > 0 for w in want) and field.connectivity == 6
        got = model.tuples(labels.clearance(records, field, boxes, keep))
        assert got == want, (name, differing(got, want))
        want = model.records_of(whole, D)
        got = model.tuples(labels.clearance(records, field))
        assert got == want, (name, differing(got, want))
        if spec == (False, False):
            least = np.array([w[3] for w in want], np.uint32)
            assert labels.freeRadius(records, field).tolist() == [model.free_radius(int(v), 32) for v in least]
        field.close()
    labels.close()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_labels_of_another_depth(built, connectivity):
    """rigid_model.random_debris at 16^3 under both connectivities, under the maps, boxes and keep mask of
    rigid_model.pose_case(32, .) taken in turn and piece 0 at the identity, over the fields of a 32^3 world"""
    vol = rigid_model.random_debris(16, 56 + connectivity)
    ids, rec = components_model.label(vol, connectivity)
    _, _, pose_maps, pose_boxes, pose_keep, base = rigid_model.pose_case(32, 56 + connectivity)
    C_ = len(rec)
    maps = [pose_maps[i % len(pose_maps)] for i in range(C_)]
    boxes = np.array([pose_boxes[i % len(pose_maps)] for i in range(C_)], np.uint32)
    keep = np.array([pose_keep[i % len(pose_maps)] for i in range(C_)], np.uint8)
    maps[0], boxes[0], keep[0] = IDENTITY, [0, 0, 0, 32, 32, 32], 1
    labels = labels_of(vol, connectivity)
    assert labels.count == C_ and labels.depth == 4
    sets = posed_cases.posed_point_sets(ids, maps, boxes, 32, keep)
    assert sum(p is not None and len(p) > 0 for p in sets) > 8
    for name, spec, D in model.fields_of(base):
        field = field_of(base, spec)
        want = model.records_of(sets, D)
        got = model.tuples(labels.clearance(affine_records(maps), field, boxes, keep))
        assert got == want, (name, differing(got, want))
        field.close()
    labels.close()


def test_every_bit_position_of_a_word(built):
    """one-voxel pieces moved to each of the 32 bit positions of an occupancy word (contact_model.bit_position_case: twice 32
    pieces, each in a column of its own), over the distance to a single solid voxel: the record is that voxel's value, at
    that voxel, as minimum, maximum and sum.  With the moved boxes and with NULL boxes."""
    ids, targets, maps, boxes, _, _ = contact_model.bit_position_case(0, 1)
    vol, _, _ = contact_model.specks()
    world = np.zeros((32, 32, 32), np.uint8)
    world[13, 21, 6] = 1
    value = ((targets - np.array([13, 21, 6])) ** 2).sum(1)
    assert len(set(tuple(t & [1, 1, 7]) for t in targets[:32])) == 32 and (value > 0).all()
    want = [(1, 0, int(v), int(v), [int(c) for c in t], int(v), [int(c) for c in t]) for v, t in zip(value, targets)]
    labels, field = labels_of(vol), field_of(world, (False, False))
    for bx in (boxes, None):
        got = labels.clearance(affine_records(maps), field, bx)
        assert model.tuples(got) == want, differing(model.tuples(got), want)
        assert np.array_equal(got["min_at"], targets) and np.array_equal(got["max_at"], targets)
        assert np.array_equal(got["min_value"], value) and np.array_equal(got["max_value"], value) and np.array_equal(got["sum"], value)
    field.close()
    labels.close()


def test_ties_across_lanes_waves_and_workgroups(built):
    """64^3: a plate of 40 x 1 x 40 voxels parallel to a floor slab, so that all 1600 voxels hold one value, and the plate
    tilted so that exactly one row of it is lowest (clearance_model.plate_case): min_at and max_at are the voxels of smallest
    dense index.  The plate's voxels lie in the items of several workgroups of the launch, and of several waves in each."""
    plate, world, maps, box = model.plate_case()
    ids, rec = components_model.label(plate, 6)
    D = distance_model.field(world)
    gx, gy = posed_cases.posed_grid(1, 64)
    assert gy == 1 and posed_cases.box_word_items(box[:3], box[3:]) > 3 * posed_cases.GROUP
    labels, field = labels_of(plate), field_of(world, (False, False))
    assert labels.count == 1
    for k, mp in enumerate(maps):
        points = posed_cases.posed_points(ids, 0, mp, box, 64)
        busy = np.flatnonzero(posed_cases.item_counts(points, box, 64))
        assert len(set((busy // posed_cases.GROUP).tolist())) > 3 and busy.max() < gx * posed_cases.GROUP       # more than one workgroup holds a voxel
        want = [model.record(points, D)]
        for bx in ([box], None):
            got = model.tuples(labels.clearance(affine_records([mp]), field, bx))
            assert got == want, (k, bx is None, got, want)
    flat = model.tuples(labels.clearance(affine_records(maps[:1]), field, [box]))[0]
    assert flat == (1600, 0, 1600 * 324, 324, [10, 20, 12], 324, [10, 20, 12])
    field.close()
    labels.close()


@pytest.mark.parametrize("S", [4, 8])
def test_a_field_of_4_cubed_and_one_of_8_cubed(built, S):
    """a 4^3 volume has two occupancy words, shared by its brick rows, though its field is dense; in 8^3 a row is one word.
    The three pieces of the contact test's 4^3 world (clearance_model.small_world_case) over the fields of random worlds and of
    a striped one, with boxes and without"""
    debris, maps, boxes = model.small_world_case(S)
    ids, rec = components_model.label(debris, 6)
    labels = labels_of(debris, 6)
    assert labels.count == 3
    rng = np.random.default_rng(9 + S)
    stripes = np.zeros((S, S, S), np.uint8)
    stripes[:, 1::2, :] = 1
    depth = 2 if S == 4 else 3
    sets = {True: posed_cases.posed_point_sets(ids, maps, boxes, S), False: posed_cases.posed_point_sets(ids, maps, None, S)}
    for world in ((rng.random((S, S, S)) < 0.3).astype(np.uint8), (rng.random((S, S, S)) < 0.6).astype(np.uint8), stripes):
        for name, spec, D in model.fields_of(world):
            field = field_of(world, spec, depth)
            assert np.array_equal(field.download(), D)
            for boxed in (True, False):
                want = model.records_of(sets[boxed], D)
                got = model.tuples(labels.clearance(affine_records(maps), field, boxes if boxed else None))
                assert got == want, (name, boxed, differing(got, want))
            field.close()
    labels.close()


def test_more_pieces_than_rows_of_the_grid(built):
    """16384 one-voxel pieces (a 32^3 checkerboard under 6-connectivity): more than the 4096 rows of the launch's grid, so a
    row takes several pieces.  Identity maps, the field of a random world, finite everywhere: record i is the field at piece
    i's voxel.  Then with a keep mask and the pieces' own boxes."""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    board = rigid_model.checkerboard(S)
    ids, rec = components_model.label(board, 6)
    C_ = len(rec)
    assert C_ == 16384 > posed_cases.GRID_ROWS
    rng = np.random.default_rng(12)
    world = (rng.random((S, S, S)) < 0.05).astype(np.uint8)
    D = distance_model.field(world)
    assert (D != NONE).all()
    p = rec["lo"].astype(np.int64)
    value = D[tuple(p.T)]
    maps = np.zeros(C_, vrc.capi.AFFINE_DTYPE)
    maps["m"][:] = stamp_model.IDENTITY[0]
    want = np.zeros(C_, vrc.capi.CLEARANCE_DTYPE)
    want["posed"], want["sum"], want["min_value"], want["max_value"], want["min_at"], want["max_at"] = 1, value, value, value, p, p
    some = list(range(0, C_, 512))
    assert model.tuples(want[some]) == [model.record(np.argwhere(ids == i), D) for i in some]
    labels, field = labels_of(board, 6), field_of(world, (False, False))
    got = labels.clearance(maps, field)
    assert got.tobytes() == want.tobytes(), differing(model.tuples(got), model.tuples(want))
    keep = (rng.random(C_) < 0.9).astype(np.uint8)
    boxes = np.concatenate([rec["lo"], rec["hi"]], 1).astype(np.uint32)
    want[keep == 0] = np.zeros(1, vrc.capi.CLEARANCE_DTYPE)[0]
    want["min_value"][keep == 0] = NONE
    got = labels.clearance(maps, field, boxes, keep)
    assert got.tobytes() == want.tobytes(), differing(model.tuples(got), model.tuples(want))
    assert (keep == 0).sum() > 1000
    field.close()
    labels.close()


def test_a_lane_takes_several_words(built):
    """posed_cases.large_case at 128^3: 257 pieces, the frame and four blocks with the whole volume for a box, so that a lane
    strides over several words of one piece (tests/test_volume_posed_cases_host.py holds the case to that).  The model's
    records come from posed_cases.large_points; the FIELD is the library's own, downloaded -- vrc_volume_distance_field of the
    case's random base world and of its own volume -- because the numpy field at 128^3 does not fit a test of a few seconds;
    tests/test_gpu_volume_distance.py holds that call to the numpy model."""
    case = posed_cases.large_case()
    points = posed_cases.large_points()
    labels = labels_of(case.vol, 6)
    assert labels.count == len(case.maps)
    records = affine_records(case.maps)
    for world in (case.base, case.vol):
        field = field_of(world, (False, False))
        D = field.download()
        want = model.records_of(points, D)
        got = model.tuples(labels.clearance(records, field, case.boxes, case.keep))
        assert got == want, differing(got, want)
        assert want[case.frame][0] > 10000 and sum(w[0] > 0 for w in want) > 150
        field.close()
    labels.close()


# ---- against the library's own calls ---------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [3, 4])
def test_conservative_advancement(built, seed):
    """what the record is for (clearance_model.advancement_case; tests/test_volume_clearance_host.py holds it to its claims):
    with rec = the clearance over the distance to the solid, a piece translated by an integer o with |o|^2 < min_value does
    not overlap the world -- vrc_rigid_contacts' overlap is 0 -- in 16 rounds of random offsets with |o|_inf <= 8, of which
    some lie within the bound and some beyond; `posed` never changes, since nothing is clipped.  And the bound is sharp: moved
    by o = q - min_at, q the nearest solid voxel to min_at, |o|^2 = min_value, the piece overlaps."""
    case = model.advancement_case(seed)
    labels, world = labels_of(case.debris, 6), volume_of(case.world)
    field = world.distanceField(False, False)
    C_ = labels.count
    assert C_ == len(case.maps)
    rec = labels.clearance(affine_records(case.maps), field)
    assert model.tuples(rec) == case.records, differing(model.tuples(rec), case.records)
    least = rec["min_value"].astype(np.int64)
    posed = rec["posed"]
    for o in case.rounds:
        moved = labels.contacts(affine_records([model.translated(mp, d) for mp, d in zip(case.maps, o)]), world)
        assert np.array_equal(moved["posed"], posed)
        within = (o ** 2).sum(1) < least
        assert within.sum() > 10 and not moved["overlap"][within].any(), np.flatnonzero(within & (moved["overlap"] > 0))
    reach = np.flatnonzero(case.reach)
    assert 2 * len(reach) >= C_
    sharp = labels.contacts(affine_records([model.translated(mp, d) for mp, d in zip(case.maps, case.last)]), world)
    assert np.array_equal(sharp["posed"], posed) and (sharp["overlap"][reach] >= 1).all()
    for v in (field, world, labels):
        v.close()


def test_device_memory_on_a_stream_and_a_map_beyond_the_limits(built):
    """keep, maps, boxes and the records in device memory on a created stream, the records filled with 0xA5 beforehand: the
    bytes are the host form's, the empty-set records of skipped pieces included; a map beyond the limits, which the host
    refuses with "piece <i>:", gives the empty-set record there; two calls give identical bytes; nothing is written around
    the records; the labels keep no scratch"""
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
    labels = labels_of(debris, 6)
    field = field_of(base, None)                                             # the travel field: NONE values as well
    with pytest.raises(vrc.VrcError, match="piece 2: m\\[0\\]"):
        labels.clearance(records, field, boxes, keep)
    all_legal = labels.clearance(legal, field, boxes, keep)
    empty = np.zeros(1, vrc.capi.CLEARANCE_DTYPE)
    empty["min_value"] = NONE
    want = all_legal.copy()
    want[[2, 4, 11]] = empty[0]
    assert all(all_legal["posed"][i] > 0 for i in (2, 4, 11))                # the three would have shown
    skipped = np.flatnonzero(keep == 0)
    assert len(skipped) > 3 and all(all_legal[i].tobytes() == empty.tobytes() for i in skipped)
    assert all_legal[5].tobytes() == empty.tobytes() == all_legal[6].tobytes()                # the empty and the inverted box
    before_bytes = labels.bytes()
    C_ = labels.count
    t_maps = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    t_boxes = torch.from_numpy(boxes.view(np.int32).copy()).cuda()
    t_keep = torch.from_numpy(keep.copy()).cuda()
    t_out = torch.from_numpy(np.full((C_ + 2) * 64, 0xA5, np.uint8)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        labels.clearanceDevice(t_maps.data_ptr(), field, t_out.data_ptr() + 64, t_boxes.data_ptr(), t_keep.data_ptr(), stream)
        vrc.capi.load().vrc_stream_synchronize(0, stream)
        once = t_out.cpu().numpy().copy()
        labels.clearanceDevice(t_maps.data_ptr(), field, t_out.data_ptr() + 64, t_boxes.data_ptr(), t_keep.data_ptr(), stream)
    twice = t_out.cpu().numpy()
    assert once.tobytes() == twice.tobytes()
    assert once[64:64 + 64 * C_].tobytes() == want.tobytes()
    assert (once[:64] == 0xA5).all() and (once[64 + 64 * C_:] == 0xA5).all()
    assert labels.bytes() == before_bytes
    # NULL boxes and NULL keep in device memory: the host form's bytes again
    whole = labels.clearance(legal, field)
    t_legal = torch.from_numpy(legal.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    labels.clearanceDevice(t_legal.data_ptr(), field, t_out.data_ptr() + 64)
    torch.cuda.synchronize()
    assert t_out.cpu().numpy()[64:64 + 64 * C_].tobytes() == whole.tobytes()
    field.close()
    labels.close()
