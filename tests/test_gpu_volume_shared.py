"""The code the volume features share (vrc_group.h, vrc_box_words.h, vrc_volume_state.h), at the smallest shapes at which
it can go wrong: the workgroup sum with idle lanes and idle waves, the two ways a destination word is written at the sizes
on either side of the shared-word rule, and the staged call with a block that has to grow and on a stream of its own behind
a device-memory edit.  Every expectation is NumPy's (the models of tests/*_model.py); every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import components_model
import distance_model
import stamp_model
import surface_model

pytestmark = pytest.mark.gpu

OPS = (stamp_model.REPLACE, stamp_model.OR, stamp_model.ANDNOT)


def random_volume(seed, depth, density):
    S = 1 << depth
    return (np.random.default_rng(seed).random((S, S, S)) < density).astype(np.uint8)


def volume_of(vol):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(int(vol.shape[0]).bit_length() - 1)
    if vol.any():
        volume.setVoxels(np.argwhere(vol))
    return volume


def apply(dst, K, op):
    if op == stamp_model.REPLACE:
        return (K != 0).astype(np.uint8)
    return (dst | K if op == stamp_model.OR else dst & (1 - K)).astype(np.uint8)


class Stream:
    def __enter__(self):
        import cpuvoxelraycaster_amd as vrc
        self.L = vrc.capi.load()
        self.h = C.c_void_p()
        vrc.capi.check(self.L.vrc_stream_create(0, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        self.L.vrc_stream_synchronize(0, self.h)
        self.L.vrc_stream_destroy(0, self.h)


@pytest.mark.parametrize("depth", [2, 4, 5])
def test_reductions(built, depth):
    """4^3: two words, 2 of 256 lanes busy.  16^3: 128 words, waves 2 and 3 add nothing.  32^3: 2048 words, 8 workgroups,
    several slots to scan, 4 groups of the labelling.  37 % full, so that the waves' partial sums differ."""
    S = 1 << depth
    vol = random_volume(3700 + depth, depth, 0.37)
    solid = int(vol.sum())
    volume = volume_of(vol)
    assert volume.solidCount() == solid
    assert list(volume.countBoxes([[0, 0, 0, S, S, S]])) == [solid]
    for closed in (True, False):
        want = surface_model.direction_counts(surface_model.faces(vol, closed))
        assert np.array_equal(volume.surfaceCount(closed), want), closed
    for to_empty in (False, True):
        field = volume.distanceField(to_empty)
        assert int(field.stats.features) == (S ** 3 - solid if to_empty else solid)
        field.close()
    # the slot scan behind the counts: ids are ranks in key order, the face list's length is the scanned total
    labels = volume.labelComponents(6)
    ids, records = components_model.label(vol, 6)
    assert labels.count == len(records)
    assert np.array_equal(labels.at(np.argwhere(vol >= 0)), ids.reshape(-1))
    labels.close()
    volume.close()


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_box_word_tail_of_copy_and_stamp(built, depth):
    """depth 2: two brick rows share a word (atomics); depth 3: n = 4, the first size with one owner per word; depth 4.  The
    box has odd bounds on every axis: first and last words are partly covered."""
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    src, dst = random_volume(4100 + depth, depth, 0.37), random_volume(4200 + depth, depth, 0.5)
    d_src, d_dst = volume_of(src), volume_of(dst)
    lo, hi = (1, 1, 1), (S - 1, S - 1, S - 1)
    size = tuple(h - l for l, h in zip(lo, hi))
    for op in OPS:
        copied, stamped = d_dst.clone(), d_dst.clone()
        copied.copyRegion(d_src, lo, size, lo, op)
        stamped.stampAffine(d_src, vrc.make_affine(*stamp_model.IDENTITY), lo, hi, op)
        got = copied.download()
        assert np.array_equal(got, stamped.download()), op
        assert np.array_equal(got, stamp_model.stamp(dst, src, *stamp_model.IDENTITY, lo, hi, op)), op
        copied.close()
        stamped.close()
    d_src.close()
    d_dst.close()


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_selected_word_tail_of_labels_and_distance(built, depth):
    vol, dst = random_volume(4300 + depth, depth, 0.37), random_volume(4400 + depth, depth, 0.5)
    volume, d_dst = volume_of(vol), volume_of(dst)
    labels, field = volume.labelComponents(6), volume.distanceField()
    ids, records = components_model.label(vol, 6)
    keep = (np.arange(len(records)) % 3 != 1).astype(np.uint8)
    by_label = components_model.select(ids, keep)
    by_distance = distance_model.select(distance_model.field(vol), 1, 2)
    assert by_label.any() and by_distance.any() and not by_label.all() and not by_distance.all()
    for op in OPS:
        work = d_dst.clone()
        labels.select(keep, work, op)
        assert np.array_equal(work.download(), apply(dst, by_label, op)), op
        work.close()
        work = d_dst.clone()
        field.select(1, 2, work, op)
        assert np.array_equal(work.download(), apply(dst, by_distance, op)), op
        work.close()
    for h in (labels, field, volume, d_dst):
        h.close()


def test_staged_calls_with_a_growing_block(built):
    """host-memory form: one item, then more items than the staging block holds, so that it is reallocated between two calls"""
    depth, S = 4, 16
    vol = random_volume(4500, depth, 0.37)
    volume = volume_of(vol)
    labels, field = volume.labelComponents(6), volume.distanceField()
    ids, _ = components_model.label(vol, 6)
    D = distance_model.field(vol)
    rng = np.random.default_rng(45)

    def queries(n):
        xyz = rng.integers(0, S, (n, 3)).astype(np.uint32)
        xyz[n // 2] = (S, 0, 0)                                  # one beyond the volume
        return xyz, (xyz < S).all(axis=1)

    def boxes(n):
        lo = rng.integers(0, S - 3, (n, 3))
        return np.concatenate([lo, lo + rng.integers(1, 4, (n, 3))], axis=1).astype(np.uint32)

    def check(n):
        xyz, inside = queries(n)
        at = tuple(np.where(inside[:, None], xyz, 0).T)
        assert np.array_equal(volume.getVoxels(xyz), np.where(inside, vol[at], 0))
        assert np.array_equal(labels.at(xyz), np.where(inside, ids[at], components_model.NO_COMPONENT))
        assert np.array_equal(field.at(xyz), np.where(inside, D[at], distance_model.NONE))
        b = boxes(n)
        want = [int(vol[x0:x1, y0:y1, z0:z1].sum()) for x0, y0, z0, x1, y1, z1 in b]
        assert list(volume.countBoxes(b)) == want

    check(1)
    cap = volume.editScratchBytes()                              # volume_of's setVoxels has sized the block: nothing else has one
    for _ in range(2):
        check(cap // 13 + 1)                                     # the block grows for get_voxels, then again for count_boxes
        grown = volume.editScratchBytes()
        assert grown > cap
        cap = grown
    for h in (labels, field, volume):
        h.close()


def test_staged_calls_in_device_memory_behind_an_edit_on_another_stream(built):
    """a device-memory edit on one stream, then the queries in device-memory form on another with no synchronisation between
    the two calls: the queries on the volume see the edit; the snapshots, taken before it, do not"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 4, 16
    vol = random_volume(4600, depth, 0.37)
    volume = volume_of(vol)
    labels, field = volume.labelComponents(6), volume.distanceField()
    ids, _ = components_model.label(vol, 6)
    D = distance_model.field(vol)
    box = np.array([[1, 3, 5, 15, 12, 11]], np.uint32)
    edited = vol.copy()
    edited[1:15, 3:12, 5:11] = 1
    n = 2 * 256 + 7                                              # more than one workgroup, the last one partly filled
    xyz = np.random.default_rng(46).integers(0, S + 1, (n, 3)).astype(np.uint32)
    inside = (xyz < S).all(axis=1)
    at = tuple(np.where(inside[:, None], xyz, 0).T)
    count_boxes = np.array([[0, 0, 0, S, S, S], [1, 1, 1, S - 1, S - 1, S - 1], [2, 4, 6, 9, 5, 16]], np.uint32)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()

    # the same two queries behind edits that take long enough to lose a race against: a whole 512^3 volume cleared and
    # filled eight times over on the first stream, read on the second
    big, B = vrc.VoxelVolume(9), 512
    big_xyz = np.random.default_rng(47).integers(0, B, (n, 3)).astype(np.uint32)
    big_boxes = np.array([[0, 0, 0, B, B, B], [B - 9, B - 7, B - 5, B, B, B], [1, 1, 1, 2, 2, B]], np.uint32)
    d_whole, d_big_xyz, d_big_boxes = dev(np.array([[0, 0, 0, B, B, B]], np.uint32)), dev(big_xyz), dev(big_boxes)
    d_big_solid = torch.full((n,), 9, dtype=torch.uint8).cuda()
    d_big_counts = torch.full((3,), -1, dtype=torch.int64).cuda()

    d_box, d_xyz, d_count_boxes = dev(box), dev(xyz), dev(count_boxes)
    d_solid = torch.full((n,), 9, dtype=torch.uint8).cuda()
    d_counts = torch.full((3,), -1, dtype=torch.int64).cuda()
    d_ids, d_d2 = torch.full((n,), 7, dtype=torch.int32).cuda(), torch.full((n,), 7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    with Stream() as first, Stream() as second:
        volume.fillBoxesDevice(1, d_box.data_ptr(), True, first)
        volume.getVoxelsDevice(n, d_xyz.data_ptr(), d_solid.data_ptr(), second)
        volume.countBoxesDevice(3, d_count_boxes.data_ptr(), d_counts.data_ptr(), second)
        labels.atDevice(n, d_xyz.data_ptr(), d_ids.data_ptr(), second)
        field.atDevice(n, d_xyz.data_ptr(), d_d2.data_ptr(), second)
        for round_ in range(16):
            big.fillBoxesDevice(1, d_whole.data_ptr(), round_ % 2 == 1, first)
        big.getVoxelsDevice(n, d_big_xyz.data_ptr(), d_big_solid.data_ptr(), second)
        big.countBoxesDevice(3, d_big_boxes.data_ptr(), d_big_counts.data_ptr(), second)
    assert not np.array_equal(edited, vol)
    assert np.array_equal(d_solid.cpu().numpy(), np.where(inside, edited[at], 0))
    want = [int(edited[x0:x1, y0:y1, z0:z1].sum()) for x0, y0, z0, x1, y1, z1 in count_boxes]
    assert d_counts.cpu().numpy().tolist() == want
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), np.where(inside, ids[at], components_model.NO_COMPONENT))
    assert np.array_equal(d_d2.cpu().numpy().view(np.uint32), np.where(inside, D[at], distance_model.NONE))
    assert np.array_equal(volume.download(), edited)
    assert (d_big_solid.cpu().numpy() == 1).all()
    assert d_big_counts.cpu().numpy().tolist() == [B ** 3, 9 * 7 * 5, B - 1]
    for h in (labels, field, volume, big):
        h.close()
