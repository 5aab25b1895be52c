"""The posed-piece kernels of vrc_rigid.hip at 128^3, where a lane takes several words of a box and carries its sums from one
iteration of its stride loop to the next, and the broad phase where it has a second workgroup (vrc_rigid_moments,
vrc_rigid_place_affine, vrc_rigid_contacts, vrc_rigid_pair_contacts, vrc_rigid_box_pair_count / vrc_rigid_box_pairs).  The cases and the
grid shapes they reach are tests/posed_cases.py's, held to their conditions in tests/test_volume_posed_cases_host.py.  The
expected values are the numpy models' (rigid_model, contact_model, pair_contact_model; the records from voxel lists, which
the host test holds against the dense form), never another GPU result.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import contact_model
import pair_contact_model
import posed_cases as cases
import rigid_model
from volume_support import Stream, affine_records, differing, tuples, volume_of

pytestmark = pytest.mark.gpu
S = 128


def labelled(case):
    """the case's volume labelled on the device, its records held to components_model.label's: that fixes the piece order"""
    medium = volume_of(case.vol)
    labels = medium.labelComponents(6)
    medium.close()
    got = labels.components()
    assert labels.count == len(case.rec)
    for field in ("first", "lo", "hi", "reserved", "voxels"):
        assert np.array_equal(got[field], case.rec[field]), field
    return labels


@pytest.fixture(scope="module")
def large(built):
    case = cases.large_case()
    labels = labelled(case)
    yield case, labels, affine_records(case.maps)
    labels.close()


@pytest.fixture(scope="module")
def scaled(built):
    case = cases.scaled_case()
    labels = labelled(case)
    yield case, labels, affine_records(case.maps)
    labels.close()


# ---- moments ---------------------------------------------------------------------------------------------------------

def test_moments_of_the_frame_and_256_blocks(large):
    """all 257 records, and a window that starts inside the list and leaves the frame out"""
    case, labels, _ = large
    want = [(n, list(s1), list(s2)) for n, s1, s2 in rigid_model.moments_fast(case.ids, 257)]
    got = [rigid_model.moments_tuple(r) for r in labels.moments()]
    assert got == want, differing(got, want)
    assert want[case.frame][0] == 23552
    first, capacity = 37, 150
    assert not first <= case.frame < first + capacity
    got = [rigid_model.moments_tuple(r) for r in labels.moments(first, capacity)]
    assert got == want[first:first + capacity], differing(got, want[first:first + capacity])


# ---- placement -------------------------------------------------------------------------------------------------------

def test_place_affine_with_the_cases_boxes(large):
    """257 rows, gx = 63: OR into a random base and ANDNOT out of a full one, with the case's boxes and keep mask"""
    import cpuvoxelraycaster_amd as vrc
    case, labels, records = large
    for op, model_op, base in ((vrc.capi.VRC_COPY_OR, rigid_model.OR, case.base), (vrc.capi.VRC_COPY_ANDNOT, rigid_model.ANDNOT, np.ones((S, S, S), np.uint8))):
        want = rigid_model.place_affine(case.ids, case.maps, case.boxes, base, model_op, case.keep)
        assert not np.array_equal(want, base)
        dst = volume_of(base)
        labels.placeAffine(records, case.boxes, dst, op, case.keep)
        got = dst.download()
        dst.close()
        assert np.array_equal(got, want), (op, int((got != want).sum()))


def test_place_affine_whole_volume_boxes_host_and_device_form(large):
    """NULL boxes and a keep mask that leaves the frame and three blocks: every kept piece walks the whole volume at gx = 63.
    The host form and the device form on a created stream"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    case, labels, records = large
    keep = np.zeros(257, np.uint8)
    keep[[case.frame] + case.whole[:3]] = 1
    want = rigid_model.place_affine(case.ids, case.maps, None, case.base, rigid_model.OR, keep)
    assert int(want.sum()) > int(case.base.sum()) + 5000
    dst = volume_of(case.base)
    labels.placeAffine(records, None, dst, vrc.capi.VRC_COPY_OR, keep)
    got = dst.download()
    dst.close()
    assert np.array_equal(got, want), int((got != want).sum())
    t_maps = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    t_keep = torch.from_numpy(keep.copy()).cuda()
    torch.cuda.synchronize()
    dst = volume_of(case.base)
    with Stream() as stream:
        labels.placeAffineDevice(t_maps.data_ptr(), dst, None, vrc.capi.VRC_COPY_OR, t_keep.data_ptr(), stream)
        got = dst.download()
    dst.close()
    assert np.array_equal(got, want), int((got != want).sum())


# ---- contacts --------------------------------------------------------------------------------------------------------

def test_contacts_against_three_worlds_and_the_walls(large):
    """all 257 records against a dense, a sparse and a rough-ground world and against an empty one, where only the faces of
    the volume count: the turned frame reaches them"""
    case, labels, records = large
    points = cases.large_points()
    empty = np.zeros((S, S, S), np.uint8)
    for name, world in contact_model.worlds(S, 3) + [("empty", empty)]:
        want = cases.contacts_of(points, world)
        assert want[case.frame][0] == 18485
        if name == "empty":
            assert want[case.frame][1] == 0 and want[case.frame][4] > 100 and all(v != 0 for v in want[case.frame][6])
        else:
            assert sum(w[1] > 0 for w in want) > 100 and sum(w[4] > 0 for w in want) > 20, name
        volume = volume_of(world)
        got = tuples(labels.contacts(records, volume, case.boxes, case.keep))
        volume.close()
        assert got == want, (name, differing(got, want))


# ---- pair contacts -----------------------------------------------------------------------------------------------------

def frame_pairs(case):
    """(frame, block) and (block, frame) over 40 blocks spread over the frame's candidates: 80 pairs"""
    mates = [b for a, b in cases.large_pairs().tolist() if a == case.frame][::5][:40]
    assert len(mates) == 40
    return np.array([(case.frame, b) for b in mates] + [(b, case.frame) for b in mates], np.uint32)


def long_pair_list(case, wanted):
    """5000 pairs: the wanted ones at seeded places -- two of them in one row of the 4096 -- among block-block candidates, some
    with a whole-volume box for a, pairs whose b or a is not kept, indices beyond the pieces and a self pair, repeated as needed:
    (the list, the places, the pieces not kept that it uses, the number of distinct other entries)"""
    rng = np.random.default_rng(17)
    between = [p for p in cases.large_pairs().tolist() if case.frame not in p]
    with_whole = [p for p in between if p[0] in case.whole][:40]
    assert len(with_whole) >= 8
    dropped = [int(i) for i in np.flatnonzero(case.keep == 0)[:4]]
    special = [(case.frame, dropped[0]), (30, dropped[1]), (dropped[2], 30), (dropped[3], case.frame), (30, 257), (257, 30), (0xFFFFFFFF, case.frame), (30, 30)]
    filler = between[::len(between) // 150][:150] + with_whole + special
    long = np.array([filler[k % len(filler)] for k in range(5000)], np.int64)
    pool = np.setdiff1d(np.arange(5000), [5, 4096 + 5])
    at = np.sort(np.concatenate([rng.choice(pool, len(wanted) - 2, replace=False), [5, 4096 + 5]]))
    long[at] = wanted
    return long.astype(np.uint32), at, dropped, len(filler)


def test_pair_contacts_one_pair_under_three_grids(large):
    """the same 80 pairs with the frame asked for as lists of one pair (gx = 272: an item a lane), as one list of 80 (gx = 204)
    and inside a list of 5000 (gy = 4096, gx = 4: 68 items a lane, rows that take two pairs) whose other entries are
    block-block candidates, pairs whose b is not kept, whose a is not kept and with an index beyond the pieces; the long list
    in device memory, where such an index gives a zero record"""
    import torch
    case, labels, records = large
    points = cases.large_points()
    wanted = frame_pairs(case)
    want = cases.pair_records_of(points, wanted, S)
    assert sum(w[1] > 0 for w in want) > 10 and sum(w[4] > 0 for w in want) > 10 and all(w[0] > 0 for w in want)
    assert cases.posed_grid(1, S)[0] == 272 and cases.posed_grid(80, S)[0] == 204 and cases.posed_grid(5000, S) == (4, 4096)
    hit = [k for k, w in enumerate(want) if w[1] > 0]
    for k in (hit[0], hit[-1], 3):                                            # frame against block, block against frame, and another
        got = tuples(labels.pairContacts(records, wanted[k:k + 1], case.boxes, 7, case.keep))
        assert got == want[k:k + 1], (k, got, want[k])
    got = tuples(labels.pairContacts(records, wanted, case.boxes, 7, case.keep))
    assert got == want, differing(got, want)
    # the long list
    long, at, dropped, fillers = long_pair_list(case, wanted)
    want_long = cases.pair_records_of(points, long, S)
    assert [want_long[k] for k in at] == want
    assert want_long[list(map(tuple, long.tolist())).index((case.frame, dropped[0]))] == (18485,) + contact_model.ZERO[1:]
    assert sum(w == contact_model.ZERO for w in want_long) >= 4 * (5000 // fillers)
    import cpuvoxelraycaster_amd as vrc
    P = len(long)
    t_maps = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    t_boxes = torch.from_numpy(case.boxes.view(np.int32).copy()).cuda()
    t_keep = torch.from_numpy(case.keep.copy()).cuda()
    t_pairs = torch.from_numpy(long.view(np.int32).copy()).cuda()
    t_out = torch.from_numpy(np.full((P + 2) * 128, 0x5A, np.uint8)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        labels.pairContactsDevice(t_maps.data_ptr(), P, t_pairs.data_ptr(), t_out.data_ptr() + 128, t_boxes.data_ptr(), 7, t_keep.data_ptr(), stream)
        vrc.capi.load().vrc_stream_synchronize(0, stream)
        raw = t_out.cpu().numpy()
    assert (raw[:128] == 0x5A).all() and (raw[128 + 128 * P:] == 0x5A).all()
    got = tuples(raw[128:128 + 128 * P].view(vrc.capi.CONTACT_DTYPE))
    assert [got[k] for k in at] == want, differing([got[k] for k in at], want)
    assert got == want_long, differing(got, want_long)


# ---- the broad phase -------------------------------------------------------------------------------------------------

def test_candidate_pairs_across_the_workgroup_boundary(large):
    """257 pieces: piece 256 is alone in the second workgroup of the broad phase.  The full list, then windows through the C
    entry points into a buffer of sentinels: the whole list, one entry, and a window that starts in the run of a piece of the
    first workgroup and ends in the run of piece 256"""
    import cpuvoxelraycaster_amd as vrc
    case, labels, _ = large
    L = vrc.capi.load()
    want = cases.large_pairs()
    got = labels.candidatePairs(case.boxes, 7, case.keep)
    assert np.array_equal(got, want), (len(got), len(want))
    count = C.c_uint64()
    vrc.capi.check(L.vrc_rigid_box_pair_count(labels._h, vrc.capi.ptr(case.keep), vrc.capi.ptr(case.boxes), 7, C.byref(count), vrc.capi.VRC_MEM_HOST, None))
    assert count.value == len(want)
    first, capacity = cases.boundary_window(want)
    inside_256 = int(np.flatnonzero(want[:, 0] == 256)[1])
    for first, capacity in ((0, len(want)), (first, 1), (inside_256, 1), (first, capacity), (first - 40, capacity + 41)):
        out = np.full((capacity + 2, 2), 0x5A5A5A5A, np.uint32)
        vrc.capi.check(L.vrc_rigid_box_pairs(labels._h, vrc.capi.ptr(case.keep), vrc.capi.ptr(case.boxes), 7, first, capacity, vrc.capi.ptr(out[1:]),
                                             vrc.capi.VRC_MEM_HOST, None))
        there = want[first:first + capacity]
        assert len(there) == capacity
        assert np.array_equal(out[1:1 + capacity], there), (first, capacity)
        assert (out[0] == 0x5A5A5A5A).all() and (out[1 + capacity:] == 0x5A5A5A5A).all(), (first, capacity)
    assert np.array_equal(labels.candidatePairs(case.boxes, 7), pair_contact_model.box_pairs(case.boxes, S))


# ---- another depth -----------------------------------------------------------------------------------------------------

def test_labels_of_64_cubed_posed_into_128_cubed(scaled):
    """129 pieces of a 64^3 labelling at scale 2 in a 128^3 world (gx = 127): placeAffine and contacts"""
    import cpuvoxelraycaster_amd as vrc
    case, labels, records = scaled
    assert labels.depth == 6 and cases.posed_grid(labels.count, S)[0] == 127
    want = rigid_model.place_affine(case.ids, case.maps, case.boxes, case.base, rigid_model.OR, case.keep)
    dst = volume_of(case.base)
    labels.placeAffine(records, case.boxes, dst, vrc.capi.VRC_COPY_OR, case.keep)
    got = dst.download()
    dst.close()
    assert int(want.sum()) > int(case.base.sum()) + 5000
    assert np.array_equal(got, want), int((got != want).sum())
    points = cases.posed_point_sets(case.ids, case.maps, case.boxes, S, case.keep)
    for name, world in (contact_model.worlds(S, 4)[0], ("empty", np.zeros((S, S, S), np.uint8))):
        want = cases.contacts_of(points, world)
        assert want[case.frame][0] > 10000 and sum(w[4] > 0 for w in want) > (50 if name == "dense" else 0)
        volume = volume_of(world)
        got = tuples(labels.contacts(records, volume, case.boxes, case.keep))
        volume.close()
        assert got == want, (name, differing(got, want))
