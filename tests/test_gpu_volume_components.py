"""Connected-component labelling on the GPU (vrc_volume_label_components, vrc_labels_*; VoxelVolume.labelComponents /
VoxelLabels).  The expected labelling is the numpy model of tests/components_model.py (held against a breadth-first search
in tests/test_volume_components_host.py), or the analytic answer where a test says so.  Every comparison is exact: the
number of components, every record, and the id at ALL S^3 coordinates plus a few outside the volume."""

import numpy as np
import pytest

import components_model as model
import flood_model
from volume_support import Stream, all_coordinates, volume_of

pytestmark = pytest.mark.gpu

NONE = model.NO_COMPONENT


def check_labels(labels, ids, rec, what):
    """count, records and at() of everything against an expected labelling"""
    S = ids.shape[0]
    assert labels.count == len(rec), (what, labels.count, len(rec))
    got = labels.components()
    assert got.dtype == model.RECORD and len(got) == len(rec)
    for field in ("first", "lo", "hi", "reserved", "voxels"):
        assert np.array_equal(got[field], rec[field]), (what, field)
    at = labels.at(all_coordinates(S))
    assert np.array_equal(at[:S ** 3].reshape(S, S, S), ids), what
    assert (at[S ** 3:] == NONE).all(), what
    assert labels.bytes() == 4 * S ** 3 + 48 * len(rec)


def check_case(vol, depth, connectivity, through_empty, what=None):
    """labels the volume on the device and holds the result against the model; returns (labels, ids, records)"""
    ids, rec = model.label(vol, connectivity, through_empty)
    volume = volume_of(vol, depth)
    labels = volume.labelComponents(connectivity, through_empty)
    volume.close()                                   # the snapshot outlives its medium
    check_labels(labels, ids, rec, what if what is not None else (depth, connectivity, through_empty))
    return labels, ids, rec


# ---- random volumes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("through_empty", [False, True])
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_random_volumes(built, depth, connectivity, through_empty):
    """M of random density around the percolation threshold (faces: 0.2 .. 0.4, all 26: 0.05 .. 0.15), as in the flood
    tests: many ragged pieces that cross brick, word and workgroup borders."""
    S = 1 << depth
    rng = np.random.default_rng(8000 + 100 * depth + connectivity + int(through_empty))
    for density in ((0.2, 0.31, 0.4) if connectivity == 6 else (0.05, 0.1, 0.15)):
        in_m = rng.random((S, S, S)) < density
        in_m[tuple(rng.integers(0, S, 3))] = True
        vol = (~in_m if through_empty else in_m).astype(np.uint8)
        labels, ids, rec = check_case(vol, depth, connectivity, through_empty, (depth, connectivity, through_empty, density))
        print(f"depth {depth} conn {connectivity} empty {through_empty} density {density}: {len(rec)} pieces, largest {int(rec['voxels'].max())}")
        assert int(rec["voxels"].sum()) == int(in_m.sum())
        labels.close()


# ---- constructed cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [10, 8, 32])
@pytest.mark.parametrize("contact", ["face", "edge", "corner"])
def test_two_boxes_in_contact(built, p, contact):
    """Two 3^3 boxes that meet across the plane(s) at p: a brick border (10), a word border (z = 7 | 8) and the border of
    a 32^3 tile (31 | 32), once per axis the contact can lie along.  A shared face joins them under both connectivities; a
    shared edge or corner only under 26."""
    depth, S = 6, 64
    for axis in range(1 if contact == "corner" else 3):
        vol = np.zeros((S, S, S), np.uint8)
        vol[p - 3:p, p - 3:p, p - 3:p] = 1
        b = [slice(p - 3, p)] * 3
        if contact == "face":
            b[axis] = slice(p, p + 3)                       # shifted along `axis` only
        elif contact == "edge":
            b = [slice(p, p + 3)] * 3
            b[axis] = slice(p - 3, p)                       # the shared edge runs along `axis`
        else:
            b = [slice(p, p + 3)] * 3
        vol[tuple(b)] = 1
        assert int(vol.sum()) == 54
        for connectivity in (6, 26):
            labels, ids, rec = check_case(vol, depth, connectivity, False, (p, contact, axis, connectivity))
            pieces = 1 if contact == "face" or connectivity == 26 else 2
            assert labels.count == pieces
            assert [int(v) for v in rec["voxels"]] == ([54] if pieces == 1 else [27, 27])
            assert tuple(rec[0]["first"]) == (p - 3, p - 3, p - 3)
            labels.close()


@pytest.mark.parametrize("depth", [2, 6])
def test_faces_are_walls(built, depth):
    """Single voxels at coordinate 0 and S - 1 of one row are two pieces, under 26 as well: nothing wraps around."""
    S = 1 << depth
    for axis in range(3):
        ends = np.full((2, 3), S // 2 + 1)
        ends[0, axis], ends[1, axis] = 0, S - 1
        vol = np.zeros((S, S, S), np.uint8)
        vol[tuple(ends.T)] = 1
        for connectivity in (6, 26):
            labels, ids, rec = check_case(vol, depth, connectivity, False, (depth, axis, connectivity))
            assert labels.count == 2 and [int(v) for v in rec["voxels"]] == [1, 1]
            assert sorted(map(tuple, rec["first"].tolist())) == sorted(map(tuple, ends.tolist()))
            labels.close()


@pytest.mark.parametrize("S", [32, 64])
def test_long_chain(built, S):
    """A one-voxel path through the whole volume is ONE piece, however long the chain of unions: analytic, no model run."""
    depth = S.bit_length() - 1
    vol, start = flood_model.serpentine(S, 2)
    xyz = np.argwhere(vol)
    rec = np.zeros(1, model.RECORD)
    rec["first"], rec["lo"], rec["hi"], rec["voxels"] = start, xyz.min(axis=0), xyz.max(axis=0) + 1, int(vol.sum())
    ids = np.where(vol != 0, 0, NONE).astype(np.uint32)
    volume = volume_of(vol, depth)
    for connectivity in (6, 26):
        labels = volume.labelComponents(connectivity)
        check_labels(labels, ids, rec, (S, connectivity))
        assert int(labels.components()["voxels"][0]) == int(vol.sum())
        labels.close()
    volume.close()


def test_checkerboard_many_pieces(built):
    """(x + y + z) & 1 at 64^3: 131072 one-voxel pieces under 6, numbered in key order -- the scan at its widest -- and one
    piece under 26.  Analytic."""
    depth, S = 6, 64
    x, y, z = np.indices((S, S, S))
    vol = ((x + y + z) & 1).astype(np.uint8)
    K = model.keys(S)
    solid = vol != 0
    ids = np.full((S, S, S), NONE, np.uint32)
    ids[solid] = np.argsort(np.argsort(K[solid])).astype(np.uint32)         # the rank of the voxel's key
    rec = np.zeros(S ** 3 // 2, model.RECORD)
    where = np.argwhere(solid)
    rec["first"][ids[solid]] = where
    rec["lo"], rec["hi"], rec["voxels"] = rec["first"], rec["first"] + 1, 1
    volume = volume_of(vol, depth)
    labels = volume.labelComponents(6)
    assert labels.count == 131072
    check_labels(labels, ids, rec, "checkerboard 6")
    got = labels.components()
    assert np.array_equal(got["lo"] + 1, got["hi"])
    labels.close()
    labels = volume.labelComponents(26)
    one = np.zeros(1, model.RECORD)
    one["first"], one["lo"], one["hi"], one["voxels"] = (1, 0, 0), (0, 0, 0), (S, S, S), S ** 3 // 2
    check_labels(labels, np.where(solid, 0, NONE).astype(np.uint32), one, "checkerboard 26")
    labels.close()
    volume.close()


@pytest.mark.parametrize("depth", [2, 3, 6])
def test_empty_and_full(built, depth):
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    S = 1 << depth
    empty = vrc.VoxelVolume(depth)
    for connectivity in (6, 26):
        labels = empty.labelComponents(connectivity)
        assert labels.count == 0 and L.vrc_labels_count(labels._h) == 0 and L.vrc_labels_depth(labels._h) == depth
        assert len(labels.components()) == 0
        assert L.vrc_labels_components(labels._h, 0, 0, None, vrc.capi.VRC_MEM_HOST, None) == 0       # capacity 0, no buffer
        assert (labels.at(all_coordinates(S)) == NONE).all()
        dst = vrc.VoxelVolume(depth)
        dst.fillBoxes([[0, 0, 0, S, 2, 1]])
        assert L.vrc_labels_select(labels._h, None, dst._h, vrc.capi.VRC_COPY_OR, vrc.capi.VRC_MEM_HOST, None) == 0
        assert dst.solidCount() == 2 * S
        assert L.vrc_labels_select(labels._h, None, dst._h, vrc.capi.VRC_COPY_REPLACE, vrc.capi.VRC_MEM_HOST, None) == 0
        assert dst.solidCount() == 0                       # K is empty
        dst.close()
        labels.close()
        # the same volume through its empty voxels, and a full one through its solid voxels: one piece, the whole volume
        full = vrc.VoxelVolume(depth)
        full.fillBoxes([[0, 0, 0, S, S, S]])
        one = np.zeros(1, model.RECORD)
        one["hi"], one["voxels"] = (S, S, S), S ** 3
        for volume, through_empty in ((empty, True), (full, False)):
            labels = volume.labelComponents(connectivity, through_empty)
            check_labels(labels, np.zeros((S, S, S), np.uint32), one, (depth, connectivity, through_empty))
            labels.close()
        labels = full.labelComponents(connectivity, True)
        assert labels.count == 0
        labels.close()
        full.close()
    empty.close()


def test_depth_2_by_hand(built):
    """4^3: two words, two brick rows to a word.  Keys: (0,0,0) 0, (1,0,0) 1, (1,1,1) 7, (0,0,3) 12, (0,2,0) 16, (0,3,0) 18,
    (2,0,0) 32, (3,3,3) 63."""
    voxels = [(0, 0, 0), (1, 0, 0), (1, 1, 1), (0, 0, 3), (0, 2, 0), (0, 3, 0), (2, 0, 0), (3, 3, 3)]
    vol = np.zeros((4, 4, 4), np.uint8)
    vol[tuple(np.array(voxels).T)] = 1
    want = {6: [0, 0, 1, 2, 3, 3, 0, 4], 26: [0, 0, 0, 1, 0, 0, 0, 2]}
    boxes = {6: [((0, 0, 0), (0, 0, 0), (3, 1, 1), 3), ((1, 1, 1), (1, 1, 1), (2, 2, 2), 1), ((0, 0, 3), (0, 0, 3), (1, 1, 4), 1),
                 ((0, 2, 0), (0, 2, 0), (1, 4, 1), 2), ((3, 3, 3), (3, 3, 3), (4, 4, 4), 1)],
             26: [((0, 0, 0), (0, 0, 0), (3, 4, 2), 6), ((0, 0, 3), (0, 0, 3), (1, 1, 4), 1), ((3, 3, 3), (3, 3, 3), (4, 4, 4), 1)]}
    for connectivity in (6, 26):
        ids = np.full((4, 4, 4), NONE, np.uint32)
        ids[tuple(np.array(voxels).T)] = want[connectivity]
        rec = np.zeros(len(boxes[connectivity]), model.RECORD)
        for r, (first, lo, hi, count) in zip(rec, boxes[connectivity]):
            r["first"], r["lo"], r["hi"], r["voxels"] = first, lo, hi, count
        labels, model_ids, _ = check_case(vol, 2, connectivity, False)
        assert np.array_equal(model_ids, ids)
        check_labels(labels, ids, rec, ("by hand", connectivity))
        labels.close()


# ---- windows ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def speckled():
    """a 32^3 volume of many pieces with its model labelling, shared and left unchanged"""
    rng = np.random.default_rng(4242)
    vol = (rng.random((32, 32, 32)) < 0.22).astype(np.uint8)
    ids, rec = model.label(vol, 6)
    assert len(rec) > 500
    return vol, ids, rec


def test_record_windows(built, speckled):
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    vol, ids, rec = speckled
    volume = volume_of(vol, 5)
    labels = volume.labelComponents(6)
    Cn = labels.count
    assert Cn == len(rec)
    canary = np.frombuffer(bytes([0xAB]) * 48, model.RECORD)[0]
    for first, capacity in [(0, 10), (0, 1), (Cn // 2 - 5, 10), (Cn - 3, 10), (Cn - 1, 1), (Cn, 4), (Cn + 5, 4), (0, Cn), (0, Cn + 9), (2 ** 40, 3)]:
        out = np.full(capacity + 3, canary, model.RECORD)
        assert L.vrc_labels_components(labels._h, first, capacity, vrc.capi.ptr(out), vrc.capi.VRC_MEM_HOST, None) == 0
        k = max(0, min(capacity, Cn - first))
        assert out[:k].tobytes() == rec[first:first + k].tobytes(), (first, capacity)
        assert out[k:].tobytes() == np.full(capacity + 3 - k, canary, model.RECORD).tobytes(), (first, capacity)
        assert labels.components(first, capacity).tobytes() == rec[first:first + k].tobytes()
    labels.close()
    volume.close()


# ---- select -----------------------------------------------------------------------------------------------------

def apply_op(dst, K, op):
    from cpuvoxelraycaster_amd import capi
    return K if op == capi.VRC_COPY_REPLACE else (dst | K) if op == capi.VRC_COPY_OR else (dst & (1 - K))


@pytest.mark.parametrize("depth", [2, 5])
def test_select(built, depth, speckled):
    import cpuvoxelraycaster_amd as vrc
    ops = (vrc.capi.VRC_COPY_REPLACE, vrc.capi.VRC_COPY_OR, vrc.capi.VRC_COPY_ANDNOT)
    S = 1 << depth
    rng = np.random.default_rng(31 + depth)
    if depth == 5:
        vol, ids, rec = speckled
    else:
        vol = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
        ids, rec = model.label(vol, 6)
    content = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    medium = volume_of(vol, depth)
    labels = medium.labelComponents(6)
    assert labels.count == len(rec)
    for trial in range(3):
        keep = (rng.random(len(rec)) < (0.5, 0.1, 0.9)[trial]).astype(np.uint8) * rng.integers(1, 256, len(rec)).astype(np.uint8)
        K = model.select(ids, keep)
        for op in ops:
            fresh = labels.select(keep, None, op)
            assert np.array_equal(fresh.download(), apply_op(np.zeros_like(vol), K, op)), (trial, op, "fresh")
            fresh.close()
            other = volume_of(content, depth)
            assert labels.select(keep, other, op) is other
            assert np.array_equal(other.download(), apply_op(content, K, op)), (trial, op, "content")
            other.close()
            itself = volume_of(vol, depth)
            own = itself.labelComponents(6)
            own.select(keep, itself, op)                    # dst is the medium the labels were made from
            assert np.array_equal(itself.download(), apply_op(vol, K, op)), (trial, op, "medium itself")
            own.close()
            itself.close()
    restored = labels.select(np.ones(len(rec), np.uint8))
    assert np.array_equal(restored.download(), vol)         # every piece kept, REPLACE: M again
    restored.close()
    with pytest.raises(ValueError):
        labels.select(np.ones(len(rec) + 1, np.uint8))
    labels.close()
    medium.close()


def test_device_memory_forms_agree_with_host_forms(built, speckled):
    import torch
    import cpuvoxelraycaster_amd as vrc
    vol, ids, rec = speckled
    S = 32
    medium = volume_of(vol, 5)
    labels = medium.labelComponents(6)
    Cn = labels.count
    rng = np.random.default_rng(77)
    keep = (rng.random(Cn) < 0.4).astype(np.uint8)
    coords = all_coordinates(S)
    t_keep = torch.from_numpy(keep).cuda()
    t_xyz = torch.from_numpy(coords.view(np.int32)).cuda()
    t_ids = torch.full((len(coords),), 5, dtype=torch.int32).cuda()
    t_rec = torch.full((48 * (Cn + 2),), 0xAB, dtype=torch.uint8).cuda()
    content = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    dsts = [volume_of(content, 5) for _ in range(3)]
    torch.cuda.synchronize()
    with Stream() as stream:
        labels.atDevice(len(coords), t_xyz.data_ptr(), t_ids.data_ptr(), stream)
        labels.componentsDevice(7, Cn, t_rec.data_ptr(), stream)          # a window that runs past the end
        for op, dst in enumerate(dsts):
            labels.selectDevice(t_keep.data_ptr(), dst, op, stream)
        downloads = [dst.download() for dst in dsts]        # ordered behind the device-memory select: it is dst's last edit
    assert np.array_equal(t_ids.cpu().numpy().view(np.uint32), labels.at(coords))
    got = t_rec.cpu().numpy()
    assert got[:48 * (Cn - 7)].tobytes() == rec[7:].tobytes() and (got[48 * (Cn - 7):] == 0xAB).all()
    K = model.select(ids, keep)
    for op, dst in enumerate(dsts):
        assert np.array_equal(downloads[op], apply_op(content, K, op)), op
        host = labels.select(keep, volume_of(content, 5), op)
        assert np.array_equal(host.download(), downloads[op])
        host.close()
        dst.close()
    labels.close()
    medium.close()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_remove_small_pieces_and_split(built, speckled, connectivity):
    vol, ids, rec = speckled
    for k in (1, 2, 5, 40, 10 ** 6):
        volume = volume_of(vol, 5)
        _, mrec = model.label(vol, connectivity)
        pieces, removed = volume.removeSmallPieces(k, connectivity)
        assert pieces == len(mrec) and removed == int((mrec["voxels"] < k).sum())
        assert np.array_equal(volume.download(), model.despeckle(vol, k, connectivity)), k
        volume.close()
    volume = volume_of(vol, 5)
    mids, mrec = model.label(vol, connectivity)
    records, pieces = volume.splitPieces(connectivity, 3)
    assert records.tobytes() == mrec.tobytes() and len(pieces) == 3
    order = np.argsort(-mrec["voxels"].astype(np.int64), kind="stable")[:3]
    for (i, piece), want in zip(pieces, order):
        assert i == int(want)
        assert np.array_equal(piece.download(), (mids == i).astype(np.uint8))
        piece.close()
    assert np.array_equal(volume.download(), vol)
    volume.close()


# ---- against the flood ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity,through_empty", [(6, False), (26, False), (6, True)])
def test_flood_from_first_gives_the_piece(built, connectivity, through_empty):
    depth, S = 6, 64
    rng = np.random.default_rng(640 + connectivity)
    density = 0.25 if connectivity == 6 else 0.1
    in_m = rng.random((S, S, S)) < density
    vol = (~in_m if through_empty else in_m).astype(np.uint8)
    medium = volume_of(vol, depth)
    labels = medium.labelComponents(connectivity, through_empty)
    rec = labels.components()
    by_size = np.argsort(-rec["voxels"].astype(np.int64), kind="stable")
    for i in (int(by_size[0]), int(by_size[len(by_size) // 2]), int(by_size[-1])):
        region = volume_of(np.zeros((1, 1, 1)), depth)
        region.setVoxels([rec[i]["first"]])
        st = region.flood(medium, connectivity, through_empty)
        keep = np.zeros(len(rec), np.uint8)
        keep[i] = 1
        piece = labels.select(keep)
        assert st.converged == 1 and st.reached == int(rec[i]["voxels"]) == piece.solidCount()
        assert np.array_equal(region.download(), piece.download())
        region.close()
        piece.close()
    labels.close()
    medium.close()


# ---- snapshot and order -----------------------------------------------------------------------------------------

def test_snapshot_survives_edits_and_labelling_is_reproducible(built, speckled):
    vol, ids, rec = speckled
    S = 32
    medium = volume_of(vol, 5)
    labels = medium.labelComponents(6)
    again = medium.labelComponents(6)
    coords = all_coordinates(S)
    assert labels.at(coords).tobytes() == again.at(coords).tobytes()
    assert labels.components().tobytes() == again.components().tobytes()
    again.close()
    medium.fillBoxes([[0, 0, 0, S, S, 16]])                 # one slab below z = 16, nothing above it
    medium.fillBoxes([[0, 0, 16, S, S, S]], False)
    slab = medium.labelComponents(6)
    assert slab.count == 1 and int(slab.components()["voxels"][0]) == 16 * S * S
    slab.close()
    check_labels(labels, ids, rec, "after edits of the medium")
    medium.close()
    check_labels(labels, ids, rec, "after the medium is gone")
    labels.close()


def test_labelling_sees_device_edits_on_a_stream(built):
    """An asynchronous device-memory edit on a caller's stream immediately before the labelling is seen by it."""
    import torch
    depth, S = 6, 64
    rng = np.random.default_rng(99)
    vol = (rng.random((S, S, S)) < 0.2).astype(np.uint8)
    medium = volume_of(vol, depth)
    extra = rng.integers(0, S, (40000, 3)).astype(np.uint32)
    boxes = np.array([[0, 30, 30, S, 32, 33], [30, 0, 7, 33, S, 9]], np.uint32)
    t_extra, t_boxes = torch.from_numpy(extra.view(np.int32)).cuda(), torch.from_numpy(boxes.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        medium.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
        medium.fillBoxesDevice(len(boxes), t_boxes.data_ptr(), True, stream)
        labels = medium.labelComponents(6)                  # nothing between the edits and the labelling
    vol[tuple(extra.astype(np.int64).T)] = 1
    for x0, y0, z0, x1, y1, z1 in boxes.astype(np.int64):
        vol[x0:x1, y0:y1, z0:z1] = 1
    assert np.array_equal(medium.download(), vol)
    ids, rec = model.label(vol, 6)
    check_labels(labels, ids, rec, "behind device edits")
    labels.close()
    medium.close()


def test_labels_against_a_volume_of_another_depth_are_refused(built):
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    small, large = vrc.VoxelVolume(5), vrc.VoxelVolume(6)
    small.fillBoxes([[1, 1, 1, 4, 4, 4]])
    labels = small.labelComponents(6)
    keep = np.ones(1, np.uint8)
    for op in (0, 1, 2):
        assert L.vrc_labels_select(labels._h, vrc.capi.ptr(keep), large._h, op, vrc.capi.VRC_MEM_HOST, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_labels_select"), L.vrc_last_error()
    with pytest.raises(vrc.VrcError, match="vrc_labels_select"):
        labels.select(keep, large)
    assert large.solidCount() == 0 and small.solidCount() == 27
    labels.close()
    small.close()
    large.close()
