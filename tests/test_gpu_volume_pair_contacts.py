"""Contacts between posed pieces, pair by pair, on the GPU (vrc_rigid_pair_contacts, vrc_rigid_box_pair_count, vrc_rigid_box_pairs;
VoxelLabels.candidatePairs / pairContacts / pairContactsDevice).  The expected records are the numpy model's
(tests/pair_contact_model.py, held against hand-written cases in tests/test_volume_pair_contacts_host.py), records written out
by hand and a closed form where a test says so, and the library's own placement and contacts where the calls must agree.
Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import components_model
import contact_model
import pair_contact_model as model
import rigid_model
import stamp_model
from volume_support import Stream, affine_records, differing, labels_of, tuples, volume_of

pytestmark = pytest.mark.gpu
IDENTITY = (list(stamp_model.IDENTITY[0]), [0, 0, 0])


def pair_list(pairs):
    return [tuple(p) for p in np.asarray(pairs).reshape(-1, 2).tolist()]


def all_pairs(n):
    return np.array([(a, b) for a in range(n) for b in range(n)], np.uint32)


def blocks(S, spec):
    """a volume with one box per (x0, x1, y0, y1, z0, z1) of spec, labelled: the boxes must not touch, and come out in
    the order of components_model.label"""
    vol = np.zeros((S, S, S), np.uint8)
    for x0, x1, y0, y1, z0, z1 in spec:
        vol[x0:x1, y0:y1, z0:z1] = 1
    ids, rec = components_model.label(vol, 6)
    assert len(rec) == len(spec)
    return vol, ids, rec


# ---- the narrow phase against the model ------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("axis,sign", contact_model.DIRECTIONS)
def test_every_bit_position_and_face_of_a_word(built, axis, sign, overlap):
    """a one-voxel piece a at each of the 32 bit positions of a word and a one-voxel piece b next to it in one direction: touch
    1 with the normal out of b; and with b on a's voxel: overlap 1.  With the moved boxes and with NULL boxes"""
    ids, maps, boxes, pairs, expected = model.bit_position_case(axis, sign, overlap)
    vol, _, _ = contact_model.specks()
    labels = labels_of(vol)
    got = tuples(labels.pairContacts(affine_records(maps), pairs, boxes))
    assert got == expected, differing(got, expected)
    got = tuples(labels.pairContacts(affine_records(maps), pairs))
    assert got == expected, differing(got, expected)
    labels.close()


@pytest.mark.parametrize("S,connectivity", [(16, 6), (16, 26), (32, 6), (32, 26)])
def test_random_debris_each_under_its_own_turned_pose(built, S, connectivity):
    """rigid_model.random_debris at 16^3 and 32^3 under both connectivities, every piece under a turn of its own, posed into
    32^3: all candidate pairs of candidatePairs -- the model's list, both orders in it -- and every field of every record; then a
    hand-made list with non-candidates, a self pair, a pair repeated and pieces that are not kept"""
    vol = rigid_model.random_debris(S, 40 + S + connectivity)
    ids, rec, maps, boxes, keep = model.turned_case(vol, connectivity, 32, S + connectivity)
    labels = labels_of(vol, connectivity)
    assert labels.count == len(rec)
    records = affine_records(maps)
    sets = contact_model.posed_sets(ids, maps, boxes, 32, keep)
    pairs = labels.candidatePairs(boxes, 5, keep)
    assert pair_list(pairs) == pair_list(model.box_pairs(boxes, 32, keep))
    assert set(pair_list(pairs)) == {(b, a) for a, b in pair_list(pairs)}
    want = model.records_of(sets, pairs, 32)
    assert sum(w[1] > 0 for w in want) > 5 and sum(w[4] > 0 for w in want) > 5
    got = tuples(labels.pairContacts(records, pairs, boxes, 5, keep))
    assert got == want, differing(got, want)
    assert labels.pairContacts(records, None, boxes, 5, keep).tobytes() == labels.pairContacts(records, pairs, boxes, 5, keep).tobytes()
    rng = np.random.default_rng(S + connectivity)
    C_ = len(rec)
    hand = np.concatenate([rng.integers(0, C_, (300, 2)), [[3, 3], [0, 0]], pairs[:40], pairs[:40][::-1], [[3, 3]]]).astype(np.uint32)
    want = model.records_of(sets, hand, 32)
    got = tuples(labels.pairContacts(records, hand, boxes, 5, keep))
    assert got == want, differing(got, want)
    labels.close()


def test_three_pieces_through_one_voxel(built):
    """three bars along x, y and z moved so that all pass through (8, 8, 8): every pair's record is that of its own two sets"""
    S = 16
    vol, ids, rec = blocks(S, [(1, 10, 1, 2, 1, 2), (12, 13, 3, 12, 12, 13), (3, 4, 13, 14, 3, 12)])
    at = np.full((3, 3), 8)
    for i, r in enumerate(rec):
        at[i, np.argmax(r["hi"].astype(np.int64) - r["lo"])] = 4             # the bar's 9 voxels from 4 to 12 along its own axis
    offsets = at - rec["lo"].astype(np.int64)
    maps = rigid_model.translation_maps(offsets)
    sets = contact_model.posed_sets(ids, maps, None, S)
    assert all(A[8, 8, 8] for A in sets)
    labels = labels_of(vol)
    pairs = all_pairs(3)
    want = model.records_of(sets, pairs, S)
    assert all(w[1] == (9 if a == b else 1) for w, (a, b) in zip(want, pair_list(pairs)))
    got = tuples(labels.pairContacts(affine_records(maps), pairs, depth=4))
    assert got == want, differing(got, want)
    labels.close()


def test_a_box_that_cuts_b(built):
    """b is a block of 6 x 6 x 12 at z 2..13 whose box ends at z = 6, in the middle of the piece and of a word; a is a slab
    lying on the cut face, z = 6: it touches b's layer z = 5 from above and finds nothing of b around itself"""
    S = 16
    vol, ids, rec = blocks(S, [(2, 8, 2, 8, 2, 14), (10, 14, 10, 14, 1, 2)])
    assert rec["voxels"][0] == 432                                            # piece 0 is the block
    offsets = np.array([[0, 0, 0], [-7, -7, 5]])                                # the slab to x, y 3..6, z = 6
    maps = rigid_model.translation_maps(offsets)
    boxes = np.array([[0, 0, 0, 16, 16, 6], [0, 0, 0, 16, 16, 16]], np.uint32)
    labels = labels_of(vol)
    pairs = np.array([[1, 0], [0, 1]], np.uint32)
    want = model.pair_contacts(ids, maps, boxes, pairs, S)
    assert want[0] == (16, 0, [0, 0, 0], [0, 0, 0], 16, [4 * (7 + 9 + 11 + 13)] * 2 + [16 * 13], [0, 0, 16])
    assert want[1][0] == 6 * 6 * 4 and want[1][4] == 16 and want[1][6] == [0, 0, -16]
    got = tuples(labels.pairContacts(affine_records(maps), pairs, boxes, 4))
    assert got == want, differing(got, want)
    whole = model.pair_contacts(ids, maps, None, pairs, S)                      # without the cut the slab is inside b
    assert whole[0][1] == 16
    assert tuples(labels.pairContacts(affine_records(maps), pairs, None, 4)) == whole
    labels.close()


def test_no_walls(built):
    """contact_model.wall_case: blocks flat against each face of the volume, in its corner and partly beyond a face, against a
    distant b: posed as vrc_rigid_contacts counts it, and no touch -- the faces are no walls here"""
    import cpuvoxelraycaster_amd as vrc
    vol, offsets = contact_model.wall_case()
    vol[15:17, 15:17, 15:17] = 1                                                # b, which stays where it is
    ids, rec = components_model.label(vol, 6)
    b = int(ids[15, 15, 15])
    offsets = np.insert(offsets, b, [0, 0, 0], 0)
    maps = rigid_model.translation_maps(offsets)
    labels, empty = labels_of(vol), vrc.VoxelVolume(5)
    pairs = np.array([(a, b) for a in range(len(rec)) if a != b], np.uint32)
    got = labels.pairContacts(affine_records(maps), pairs)
    want = model.pair_contacts(ids, maps, None, pairs, 32)
    assert tuples(got) == want, differing(tuples(got), want)
    walled = labels.contacts(affine_records(maps), empty)
    others = [a for a in range(len(rec)) if a != b]
    assert (got["posed"] == walled["posed"][others]).all() and sorted(got["posed"].tolist()) == [18] + [27] * 7
    assert not got["touch"].any() and not got["overlap"].any() and (walled["touch"][others] > 0).all()
    empty.close()
    labels.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_posed_volumes_of_4_and_8_cubed(built, depth):
    """a posed volume of 4^3 has two occupancy words, shared by its brick rows; 8^3 has one word a row.  Three pieces of a
    16^3 labelling shrunk by 4 or 2 (point sampling), with boxes and without: all nine pairs"""
    S, Sd = 16, 1 << depth
    debris = np.zeros((S, S, S), np.uint8)
    debris[0:9, 0:16, 0:7] = 1
    debris[10:16, 2:14, 0:16] = 1
    debris[0:8, 3:9, 9:16] = 1
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 3
    k = S // Sd
    shrunk = [k * stamp_model.ONE if a == b else 0 for a in range(3) for b in range(3)]
    turned = [0, k * stamp_model.ONE, 0, -k * stamp_model.ONE, 0, 0, 0, 0, k * stamp_model.ONE]
    maps = [(shrunk, [0, 0, 0]), (shrunk, [-(3 << 17), 1 << 16, 0]), (turned, [0, 16 << 17, 5 << 15])]
    boxes = np.array([[0, 0, 0, Sd, Sd, Sd], [1, 0, 0, Sd, Sd - 1, Sd], [0, 0, 1, Sd, Sd, 0xFFFFFFFF]], np.uint32)
    labels = labels_of(debris, 6)
    pairs = all_pairs(3)
    seen = set()
    for bx in (boxes, None):
        want = model.pair_contacts(ids, maps, bx, pairs, Sd)
        got = tuples(labels.pairContacts(affine_records(maps), pairs, bx, depth))
        assert got == want, (bx is None, differing(got, want))
        seen.update(i for i, w in enumerate(want) if w[1] and w[4])
    assert seen == {2, 6}                                                      # pieces 0 and 2 both overlap and touch, either way round
    labels.close()


def test_more_pairs_than_rows_of_the_grid(built):
    """5000 pairs over the 64 one-voxel pieces of contact_model.specks, moved at random inside 12^3 so that many meet: more
    than the 4096 rows of the launch's grid, so a row takes several pairs.  The records by a restatement for one-voxel pieces
    in whole arrays, and that restatement against the model on every 16th pair"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    vol, ids, rec = contact_model.specks(S)
    rng = np.random.default_rng(21)
    at = rng.integers(10, 14, (64, 3))
    offsets = at - rec["lo"].astype(np.int64)
    maps, boxes = rigid_model.translation_maps(offsets), rigid_model.moved_boxes(rec, offsets, S)
    pairs = rng.integers(0, 64, (5000, 2)).astype(np.uint32)
    pa, pb = at[pairs[:, 0]], at[pairs[:, 1]]
    d = pb - pa
    same, next_to = (d == 0).all(1), np.abs(d).sum(1) == 1
    want = np.zeros(5000, vrc.capi.CONTACT_DTYPE)
    want["posed"], want["overlap"], want["touch"] = 1, same, next_to
    want["overlap_s1"], want["touch_s1"] = (2 * pa + 1) * same[:, None], (2 * pa + 1) * next_to[:, None]
    want["touch_n"] = -d * next_to[:, None]                                     # b at p + e: n = -e
    some = list(range(0, 5000, 16))
    assert tuples(want[some]) == model.pair_contacts(ids, maps, boxes, pairs[some], S)
    assert same.sum() > 50 and next_to.sum() > 200
    labels = labels_of(vol)
    got = labels.pairContacts(affine_records(maps), pairs, boxes)
    assert got.tobytes() == want.tobytes(), differing(tuples(got), tuples(want))
    labels.close()


def test_keep_and_an_inverted_box_on_either_side(built):
    vol, offsets = model.inner_blocks()
    ids, rec = components_model.label(vol, 6)
    n = len(rec)
    maps = rigid_model.translation_maps(offsets)
    boxes = rigid_model.moved_boxes(rec, offsets, 32)
    boxes[2] = [9, 0, 0, 4, 32, 32]                                             # inverted
    boxes[4, 3:] = boxes[4, :3]                                                 # empty
    keep = np.ones(n, np.uint8)
    keep[1] = 0
    labels = labels_of(vol)
    pairs = all_pairs(n)
    want = model.pair_contacts(ids, maps, boxes, pairs, 32, keep)
    for (a, b), w in zip(pair_list(pairs), want):
        if a in (1, 2, 4):
            assert w == model.ZERO
        elif b in (1, 2, 4):
            assert w[0] > 0 and w[1:] == model.ZERO[1:]
    assert sum(w[1] > 0 for w in want) > 4
    got = tuples(labels.pairContacts(affine_records(maps), pairs, boxes, None, keep))
    assert got == want, differing(got, want)
    labels.close()


def test_device_memory_on_a_stream_and_what_the_host_cannot_see(built):
    """keep, maps, boxes, pairs and the records in device memory on a created stream: a map beyond the limits and a pair index
    beyond the pieces give all-zero records and leave the others as the host-memory call has them; two calls give identical
    bytes; nothing is written around the records; the labels keep no scratch"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    vol, offsets = model.inner_blocks()
    ids, rec = components_model.label(vol, 6)
    n = len(rec)
    maps = rigid_model.translation_maps(offsets)
    boxes = rigid_model.moved_boxes(rec, offsets, 32)
    keep = np.ones(n, np.uint8)
    labels, other = labels_of(vol), vrc.VoxelVolume(5)
    legal = affine_records(maps)
    pairs = np.concatenate([all_pairs(n), [[0, n], [n, 0], [0xFFFFFFFF, 1]]]).astype(np.uint32)
    P = len(pairs)
    host = labels.pairContacts(legal, pairs[:n * n], boxes, 5, keep)
    assert tuples(host) == model.pair_contacts(ids, maps, boxes, pairs[:n * n], 32, keep)
    records = legal.copy()
    records["m"][3][0] = (1 << 20) + 1
    with pytest.raises(vrc.VrcError, match="piece 3: m\\[0\\]"):
        labels.pairContacts(records, pairs[:n * n], boxes, 5, keep)
    want = np.zeros(P, vrc.capi.CONTACT_DTYPE)
    want[:n * n] = host
    for k, (a, b) in enumerate(pair_list(pairs[:n * n])):
        if a == 3:
            want[k] = np.zeros(1, vrc.capi.CONTACT_DTYPE)[0]
        elif b == 3:
            want[k] = np.zeros(1, vrc.capi.CONTACT_DTYPE)[0]
            want[k]["posed"] = host[k]["posed"]
    before_bytes, before_scratch = labels.bytes(), other.editScratchBytes()
    t_maps = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    t_boxes = torch.from_numpy(boxes.view(np.int32).copy()).cuda()
    t_keep = torch.from_numpy(keep.copy()).cuda()
    t_pairs = torch.from_numpy(pairs.view(np.int32).copy()).cuda()
    t_out = torch.from_numpy(np.full((P + 2) * 128, 0x5A, np.uint8)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        labels.pairContactsDevice(t_maps.data_ptr(), P, t_pairs.data_ptr(), t_out.data_ptr() + 128, t_boxes.data_ptr(), 5, t_keep.data_ptr(), stream)
        vrc.capi.load().vrc_stream_synchronize(0, stream)
        once = t_out.cpu().numpy().copy()
        labels.pairContactsDevice(t_maps.data_ptr(), P, t_pairs.data_ptr(), t_out.data_ptr() + 128, t_boxes.data_ptr(), 5, t_keep.data_ptr(), stream)
    twice = t_out.cpu().numpy()
    assert once.tobytes() == twice.tobytes()
    assert once[128:128 + 128 * P].tobytes() == want.tobytes()
    assert (once[:128] == 0x5A).all() and (once[128 + 128 * P:] == 0x5A).all()
    # the broad phase in device memory: the same list, and nothing beyond it
    count = C.c_uint64()
    L = vrc.capi.load()
    vrc.capi.check(L.vrc_rigid_box_pair_count(labels._h, vrc.capi.ptr(t_keep.data_ptr()), vrc.capi.ptr(t_boxes.data_ptr()), 5, C.byref(count),
                                              vrc.capi.VRC_MEM_DEVICE, None))
    listed = labels.candidatePairs(boxes, 5, keep)
    assert count.value == len(listed) > 4
    t_list = torch.from_numpy(np.full((len(listed) + 2) * 2, 0x5A5A5A5A, np.uint32).view(np.int32)).cuda()
    with Stream() as stream:
        vrc.capi.check(L.vrc_rigid_box_pairs(labels._h, vrc.capi.ptr(t_keep.data_ptr()), vrc.capi.ptr(t_boxes.data_ptr()), 5, 0, len(listed) + 1,
                                             vrc.capi.ptr(t_list.data_ptr() + 8), vrc.capi.VRC_MEM_DEVICE, stream))
    back = t_list.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert np.array_equal(back[1:-1], listed) and (back[0] == 0x5A5A5A5A).all() and (back[-1] == 0x5A5A5A5A).all()
    assert labels.bytes() == before_bytes and other.editScratchBytes() == before_scratch
    other.close()
    labels.close()


def test_a_bad_index_in_host_memory(built):
    import cpuvoxelraycaster_amd as vrc
    vol, offsets = model.inner_blocks()
    labels = labels_of(vol)
    n = labels.count
    maps = affine_records(rigid_model.translation_maps(offsets))
    pairs = np.array([[0, 1], [1, 2], [2, n], [n + 5, 0]], np.uint32)
    out = np.full(4, 9, vrc.capi.CONTACT_DTYPE)
    L = vrc.capi.load()
    rc = L.vrc_rigid_pair_contacts(labels._h, None, vrc.capi.ptr(maps), None, 5, 4, vrc.capi.ptr(pairs), vrc.capi.ptr(out), vrc.capi.VRC_MEM_HOST, None)
    assert rc == -1 and b"pair 2" in L.vrc_last_error(), L.vrc_last_error()
    assert out.tobytes() == np.full(4, 9, vrc.capi.CONTACT_DTYPE).tobytes()
    with pytest.raises(vrc.VrcError, match="pair 2: piece %d of %d components" % (n, n)):
        labels.pairContacts(maps, pairs)
    labels.close()


def test_totals_beyond_32_bits(built):
    """256^3, one full-cube piece at the identity pose against itself -- the self pair, from which nothing is excluded: every
    voxel overlaps, and the sum of c is S^4 = 2^32 per axis, the smallest cube at which a sum leaves 32 bits.  Without walls
    the voxels of the six faces have an open neighbour: the normals sum to zero by symmetry.  Closed form, one pair only"""
    import cpuvoxelraycaster_amd as vrc
    S = 256
    medium = vrc.VoxelVolume(8)
    medium.fillBoxes([[0, 0, 0, S, S, S]])
    labels = medium.labelComponents(6)
    assert labels.count == 1
    n, s1, _ = rigid_model.solid_cube_moments(S)
    assert n == 1 << 24 and s1 == [1 << 32] * 3
    got = tuples(labels.pairContacts(affine_records([IDENTITY]), [[0, 0]]))
    assert got == [(n, n, s1, [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])]
    # one layer of it: the box x < 1 keeps S^2 voxels at c_x = 1 on both sides of the pair.  Their x neighbours are beyond the
    # volume and beyond box b, so both read 0; the y and z normals of the layer's rim cancel
    got = tuples(labels.pairContacts(affine_records([IDENTITY]), [[0, 0]], np.array([[0, 0, 0, 1, S, S]], np.uint32)))
    assert got == [(S * S, S * S, [S * S, S ** 3, S ** 3], [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])]
    medium.close()
    labels.close()


# ---- against the library's own calls ---------------------------------------------------------------------------------

def test_pair_contacts_are_contacts_against_the_placement_of_b(built):
    """for pieces away from the faces, pairContacts of (a, b) equals byte for byte contacts of a alone against placeAffine of b
    alone: no model in between"""
    import cpuvoxelraycaster_amd as vrc
    vol = rigid_model.random_debris(16, 62)
    ids, rec, maps, boxes, keep = model.turned_case(vol, 6, 32, 22)
    inner = [i for i in range(len(rec)) if (boxes[i, :3] >= 1).all() and (boxes[i, 3:] <= 31).all() and (boxes[i, 3:] > boxes[i, :3]).all()]
    labels = labels_of(vol)
    records = affine_records(maps)
    pairs = np.array([p for p in pair_list(labels.candidatePairs(boxes, 5)) if p[0] in inner and p[1] in inner], np.uint32)
    got = labels.pairContacts(records, pairs, boxes, 5)
    assert (got["overlap"] > 0).sum() > 3 and (got["touch"] > 0).sum() > 10
    checked = 0
    for b in sorted(set(pairs[:, 1].tolist()))[:12]:
        only = np.zeros(labels.count, np.uint8)
        only[b] = 1
        world = vrc.VoxelVolume(5)
        labels.placeAffine(records, boxes, world, vrc.capi.VRC_COPY_OR, only)
        against = labels.contacts(records, world, boxes)
        for k in np.flatnonzero(pairs[:, 1] == b):
            assert got[k].tobytes() == against[pairs[k, 0]].tobytes(), (pairs[k], got[k], against[pairs[k, 0]])
            checked += 1
        world.close()
    assert checked > 50
    labels.close()


# ---- the broad phase -----------------------------------------------------------------------------------------------

def test_candidate_pairs(built):
    """random boxes with a keep mask; boxes that meet at a face, an edge and a corner (candidates) and one voxel apart (none);
    windows that start and end inside one a's run, first beyond the count, a capacity beyond the end; C = 1"""
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    rng = np.random.default_rng(4)
    C_ = 300
    lo = rng.integers(0, 28, (C_, 3))
    boxes = np.concatenate([lo, lo + rng.integers(-1, 9, (C_, 3))], 1).astype(np.uint32)
    boxes[:9] = [[0, 0, 0, 4, 4, 4], [4, 0, 0, 8, 4, 4], [4, 4, 0, 8, 8, 4], [4, 4, 4, 8, 8, 8], [9, 0, 0, 12, 4, 4], [6, 6, 6, 6, 9, 9],
                 [9, 9, 9, 7, 12, 12], [30, 30, 30, 40, 40, 40], [32, 0, 0, 36, 4, 4]]
    keep = (rng.random(C_) < 0.8).astype(np.uint8)
    keep[:9] = 1
    vol = np.zeros((32, 32, 32), np.uint8)
    vol[::4, ::4, 0:31:2] = 1                                                   # 1024 one-voxel pieces; only their number matters
    vol.reshape(-1)[np.flatnonzero(vol.reshape(-1))[C_:]] = 0
    labels = labels_of(vol)
    assert labels.count == C_
    want = model.box_pairs(boxes, 32, keep)
    got = labels.candidatePairs(boxes, 5, keep)
    assert len(want) > 300 and np.array_equal(got, want)
    first9 = [p for p in pair_list(got) if p[0] < 9 and p[1] < 9]
    assert first9 == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, 3), (3, 0), (3, 1), (3, 2)]
    assert np.array_equal(labels.candidatePairs(boxes, 5), model.box_pairs(boxes, 32))
    assert np.array_equal(labels.candidatePairs(boxes, 4, keep), model.box_pairs(boxes, 16, keep))      # another clipping
    runs = np.flatnonzero(np.diff(want[:, 0]) == 0)                             # k with entries k and k + 1 in one a's run
    k = int(runs[len(runs) // 2])
    for first, capacity in ((k, 1), (k, 2), (k - 3, 5), (0, 7), (len(want) - 2, 10), (len(want), 4), (len(want) + 100, 4), (5, 0)):
        out = np.full((capacity + 2, 2), 0x5A5A5A5A, np.uint32)
        vrc.capi.check(L.vrc_rigid_box_pairs(labels._h, vrc.capi.ptr(keep), vrc.capi.ptr(boxes), 5, first, capacity,
                                             vrc.capi.ptr(out[1:]) if capacity else None, vrc.capi.VRC_MEM_HOST, None))
        there = want[first:first + capacity]
        assert np.array_equal(out[1:1 + len(there)], there), (first, capacity)
        assert (out[0] == 0x5A5A5A5A).all() and (out[1 + len(there):] == 0x5A5A5A5A).all(), (first, capacity)
    labels.close()
    one = np.zeros((16, 16, 16), np.uint8)
    one[3, 3, 3] = 1
    labels = labels_of(one)
    assert labels.candidatePairs([[0, 0, 0, 16, 16, 16]]).shape == (0, 2)
    assert len(labels.pairContacts(affine_records([IDENTITY]), None, [[0, 0, 0, 16, 16, 16]])) == 0
    labels.close()


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_fracture_turn_and_collide(built):
    """a block at 32^3 fractured around a handful of sites.  At the identity pose, with the record boxes, no pair overlaps and
    every pair of shards that share a face touches; with every shard turned a little about its own centre the candidate pairs
    and their records are the model's.  The calls leave no scratch behind"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[6:26, 8:24, 7:25] = 1
    sites = np.array([[8, 10, 9], [22, 12, 20], [15, 20, 12], [12, 14, 22], [24, 21, 10], [17, 9, 16]], np.int32)
    medium = volume_of(vol)
    labels = medium.fracture(sites)
    before_bytes, before_scratch = labels.bytes(), medium.editScratchBytes()
    ids = np.full((S, S, S), model.NONE, np.uint32)
    xyz = np.argwhere(vol).astype(np.uint32)
    ids[tuple(xyz.T)] = labels.at(xyz)
    rec = labels.components()
    n = labels.count
    assert n >= len(sites)
    still = [IDENTITY] * n
    boxes = np.concatenate([rec["lo"], rec["hi"]], 1).astype(np.uint32)
    pairs = labels.candidatePairs(boxes)
    assert np.array_equal(pairs, model.box_pairs(boxes, S))
    got = labels.pairContacts(affine_records(still), pairs, boxes)
    assert tuples(got) == model.pair_contacts(ids, still, boxes, pairs, S)
    assert not got["overlap"].any()
    share = set()
    for axis in range(3):
        lower, upper = [np.take(ids, range(k, S - 1 + k), axis) for k in (0, 1)]
        for a, b in zip(lower[(lower != upper) & (lower != model.NONE) & (upper != model.NONE)], upper[(lower != upper) & (lower != model.NONE) & (upper != model.NONE)]):
            share.update([(int(a), int(b)), (int(b), int(a))])
    assert len(share) >= 10 and share == {p for p, r in zip(pair_list(pairs), got) if r["touch"] > 0}
    _, _, maps, turned_boxes, _ = turned_from(ids, rec, S)
    pairs = labels.candidatePairs(turned_boxes)
    assert np.array_equal(pairs, model.box_pairs(turned_boxes, S))
    want = model.pair_contacts(ids, maps, turned_boxes, pairs, S)
    got = tuples(labels.pairContacts(affine_records(maps), None, turned_boxes))
    assert got == want, differing(got, want)
    assert sum(w[1] > 0 for w in want) > 4 and sum(w[4] > 0 for w in want) > 4
    assert labels.bytes() == before_bytes and medium.editScratchBytes() == before_scratch
    medium.close()
    labels.close()


def turned_from(ids, rec, S):
    """every piece of a given labelling turned a little about its own box centre and left where it is"""
    rng = np.random.default_rng(8)
    maps, boxes = [], np.zeros((len(rec), 6), np.uint32)
    for i, r in enumerate(rec):
        lo, hi = r["lo"].astype(np.float64), r["hi"].astype(np.float64)
        centre = (lo + hi) / 2
        ax, ay = rng.uniform(-0.15, 0.15, 2)
        cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
        R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        inv = R.T
        maps.append(([int(round(v * stamp_model.ONE)) for v in inv.reshape(9)], [int(round(v * (1 << 17))) for v in centre - inv @ centre]))
        half = np.abs(R) @ ((hi - lo) / 2) + 1
        boxes[i, :3] = np.clip(np.floor(centre - half), 0, S)
        boxes[i, 3:] = np.clip(np.ceil(centre + half), 0, S)
    return ids, rec, maps, boxes, None
