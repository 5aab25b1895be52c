"""The code the volume features share (vrc_group.h, vrc_box_words.h, vrc_volume_state.h), at the smallest shapes at which
it can go wrong: the workgroup sum with idle lanes and idle waves, the two ways a destination word is written at the sizes
on either side of the shared-word rule, and the staged call with a block that has to grow and on a stream of its own behind
a device-memory edit -- of the volume it writes, and of the second volume it only reads --, with every combination of
optional parts in a block of the call's own, and with a part that goes up and comes back; the window of the emit prologue the three lists share (vrc_list.h) and the paged fetch of the Python
wrapper.  Every expectation is NumPy's (the models of tests/*_model.py); every comparison is exact."""
import functools

import numpy as np
import pytest

import cells_model
import columns_model
import components_model
import contact_model
import delta_model
import distance_model
import fall_model
import fracture_model
import levels_model
import morph_model
import rect_cases
import rect_model
import rigid_model
import stamp_model
import surface_model
import travel_model
import voxels_model
from volume_support import Ballast, Stream, affine_records, device_words, event_on, volume_of

pytestmark = pytest.mark.gpu

OPS = (stamp_model.REPLACE, stamp_model.OR, stamp_model.ANDNOT)


def random_volume(seed, depth, density):
    S = 1 << depth
    return (np.random.default_rng(seed).random((S, S, S)) < density).astype(np.uint8)


def apply(dst, K, op):
    if op == stamp_model.REPLACE:
        return (K != 0).astype(np.uint8)
    return (dst | K if op == stamp_model.OR else dst & (1 - K)).astype(np.uint8)


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


def test_two_volume_calls_behind_an_edit_of_the_source_on_another_stream(built):
    """The second volume of the call frame: a device-memory fill of src on one stream -- behind the ballast (volume_support:
    whole-volume fills of a 512^3 volume) on that stream, so that it is late, which is asserted -- then, with no
    synchronisation, every call that only reads src on another stream,
    each into a destination of its own: all of them see the fill.  16^3 is the smallest size with more than one word per row
    and a brick that is not shared.  Such a test can show a missing wait; it cannot prove a present one."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 4, 16
    vol, base = random_volume(4700, depth, 0.37), random_volume(4701, depth, 0.5)
    base_up, base_down = random_volume(4702, depth + 1, 0.5), random_volume(4703, depth - 2, 0.5)
    edited = vol.copy()
    edited[1:15, 3:12, 5:11] = 1
    assert not np.array_equal(edited, vol)
    element = morph_model.box(3, 3, 3)
    birth, survive = sum(1 << c for c in range(9, 27)), sum(1 << c for c in range(6, 27))
    any_lo, any_hi = levels_model.count_range("any", 2)
    whole = ((0, 0, 0), (S, S, S))

    src, ballast = volume_of(vol), Ballast()
    copied, stamped, selected, stepped, morphed = (volume_of(base) for _ in range(5))
    up, down = volume_of(base_up), volume_of(base_down)
    d_box, d_element = device_words(np.array([[1, 3, 5, 15, 12, 11]], np.uint32)), device_words(element)
    torch.cuda.synchronize()
    with Stream() as first, Stream() as second:
        ballast.enqueue(first)
        src.fillBoxesDevice(1, d_box.data_ptr(), True, first)
        late = event_on(first)
        copied.copyRegion(src, whole[0], whole[1], whole[0], stamp_model.OR, second)
        stamped.stampAffine(src, vrc.make_affine(*stamp_model.IDENTITY), None, None, stamp_model.REPLACE, second)
        src.selectColumns(4, 1, 3, columns_model.SOLID, selected, stamp_model.ANDNOT, second)
        src.cellStep(birth, survive, 26, False, stepped, False, second)
        src.morphDevice(morphed, morph_model.DILATE, len(element), d_element.data_ptr(), stream=second)
        src.expandInto(up, stamp_model.OR, second)
        src.reduceInto(down, any_lo, any_hi, stamp_model.REPLACE, second)
        assert not late.query(), "the fill of src was not late: it had landed before the last call was enqueued"
    assert np.array_equal(src.download(), edited)
    assert np.array_equal(copied.download(), stamp_model.stamp(base, edited, *stamp_model.IDENTITY, *whole, stamp_model.OR))
    assert np.array_equal(stamped.download(), stamp_model.stamp(base, edited, *stamp_model.IDENTITY, *whole, stamp_model.REPLACE))
    assert np.array_equal(selected.download(), columns_model.select(base, edited, 4, 1, 3, columns_model.SOLID, stamp_model.ANDNOT))
    assert np.array_equal(stepped.download(), cells_model.step(edited, birth, survive, 26, 0)[0])
    assert np.array_equal(morphed.download(), morph_model.apply(base, edited, morph_model.DILATE, element))
    assert np.array_equal(up.download(), levels_model.expand(base_up, edited, stamp_model.OR))
    assert np.array_equal(down.download(), levels_model.reduce(base_down, edited, any_lo, any_hi, stamp_model.REPLACE))
    assert int(ballast.big.solidCount()) == 0                    # the ballast's last fill cleared it
    for h in (src, ballast, copied, stamped, selected, stepped, morphed, up, down):
        h.close()


# ---- the calls with several parts: labels, keep bytes, offsets, maps, boxes, records -----------------------------------

def scattered_blocks(extra=0):
    """16^3: seven small blocks (and `extra` more specks) that touch nowhere, so 7 + extra pieces under 6-connectivity -- no
    multiple of 16, so the keep bytes end off any alignment"""
    vol = np.zeros((16, 16, 16), np.uint8)
    for (x, y, z), (a, b, c) in [((1, 1, 1), (3, 2, 1)), ((6, 1, 2), (1, 1, 1)), ((11, 2, 1), (2, 3, 2)), ((1, 7, 6), (2, 2, 3)),
                                 ((6, 6, 11), (3, 1, 2)), ((11, 11, 6), (1, 3, 1)), ((2, 11, 11), (2, 2, 2))]:
        vol[x:x + a, y:y + b, z:z + c] = 1
    for k in range(extra):
        vol[15, 2 * (k % 8), 2 * (k // 8)] = 1
    return vol


@functools.lru_cache(maxsize=None)
def piece_case():
    """the scene of the multi-part tests and everything the model says about it, computed once and never written again"""
    rng = np.random.default_rng(4700)
    vol = scattered_blocks()
    ids, records = components_model.label(vol, 6)
    count = len(records)
    assert count == 7
    offsets = rng.integers(-3, 4, (count, 3)).astype(np.int32)
    maps = rigid_model.translation_maps(offsets)
    boxes = rigid_model.moved_boxes(records, offsets, 16)
    keep = (np.arange(count) % 3 != 1).astype(np.uint8)
    base = (rng.random((16, 16, 16)) < 0.3).astype(np.uint8)
    world = (rng.random((16, 16, 16)) < 0.2).astype(np.uint8)
    world[:, :3, :] = 1
    want = {"moments": rigid_model.moments(ids, count)}
    for use_keep in (False, True):
        k = keep if use_keep else None
        want["select", use_keep] = apply(base, components_model.select(ids, keep if use_keep else np.ones(count, np.uint8)), stamp_model.OR)
        want["place", use_keep] = fall_model.place(ids, offsets, base, True, k)
        for use_boxes in (False, True):
            b = boxes if use_boxes else None
            want["placeAffine", use_keep, use_boxes] = rigid_model.place_affine(ids, maps, b, base, rigid_model.OR, k)
            want["contacts", use_keep, use_boxes] = contact_model.contacts(ids, maps, b, world, k)
    for a in (vol, offsets, boxes, keep, base, world):
        a.setflags(write=False)
    return vol, offsets, maps, boxes, keep, base, world, want


def device_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("use_boxes", [False, True])
@pytest.mark.parametrize("use_keep", [False, True])
def test_multi_part_calls_in_host_and_device_form(built, use_keep, use_boxes):
    """select, place, placeAffine, contacts and moments once with their lists in host memory (staged in one block, every
    present part at an offset of its own) and once in device memory on a created stream, keep and boxes present and absent:
    the volumes and records of the two forms are equal and are the model's"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    vol, offsets, maps, boxes, keep, base, world, want = piece_case()
    medium, d_world = volume_of(vol), volume_of(world)
    labels = medium.labelComponents(6)
    count = labels.count
    assert count == 7
    records = affine_records(maps)
    keep_all = np.ones(count, np.uint8)
    k, b = (keep if use_keep else None), (boxes if use_boxes else None)

    host = {}
    for name, run in (("select", lambda dst: labels.select(keep if use_keep else keep_all, dst, stamp_model.OR)),
                      ("place", lambda dst: labels.place(offsets, dst, stamp_model.OR, k)),
                      ("placeAffine", lambda dst: labels.placeAffine(records, b, dst, stamp_model.OR, k))):
        dst = volume_of(base)
        run(dst)
        host[name] = dst.download()
        dst.close()
    host["contacts"] = labels.contacts(records, d_world, b, k)
    host["moments"] = labels.moments()

    t_keep, t_keep_all, t_offsets = device_bytes(keep), device_bytes(keep_all), device_bytes(offsets)
    t_maps, t_boxes = device_bytes(records), device_bytes(boxes)
    t_contacts = torch.full((count * 128,), 0x5A, dtype=torch.uint8).cuda()
    t_moments = torch.full((count * 80,), 0x5A, dtype=torch.uint8).cuda()
    p_keep = t_keep.data_ptr() if use_keep else None
    p_boxes = t_boxes.data_ptr() if use_boxes else None
    dsts = {name: volume_of(base) for name in ("select", "place", "placeAffine")}
    torch.cuda.synchronize()
    with Stream() as stream:
        labels.selectDevice(t_keep.data_ptr() if use_keep else t_keep_all.data_ptr(), dsts["select"], stamp_model.OR, stream)
        labels.placeDevice(t_offsets.data_ptr(), dsts["place"], stamp_model.OR, p_keep, stream)
        labels.placeAffineDevice(t_maps.data_ptr(), dsts["placeAffine"], p_boxes, stamp_model.OR, p_keep, stream)
        labels.contactsDevice(t_maps.data_ptr(), d_world, t_contacts.data_ptr(), p_boxes, p_keep, stream)
        labels.momentsDevice(0, count, t_moments.data_ptr(), stream)
    device = {name: dst.download() for name, dst in dsts.items()}
    device["contacts"] = t_contacts.cpu().numpy().view(vrc.capi.CONTACT_DTYPE)
    device["moments"] = t_moments.cpu().numpy().view(vrc.capi.MOMENTS_DTYPE)

    for name in ("select", "place"):
        assert np.array_equal(host[name], want[name, use_keep]), name
        assert np.array_equal(device[name], host[name]), name
    assert np.array_equal(host["placeAffine"], want["placeAffine", use_keep, use_boxes])
    assert np.array_equal(device["placeAffine"], host["placeAffine"])
    assert [contact_model.record_tuple(r) for r in host["contacts"]] == want["contacts", use_keep, use_boxes]
    assert device["contacts"].tobytes() == host["contacts"].tobytes()
    assert [rigid_model.moments_tuple(r) for r in host["moments"]] == want["moments"]
    assert device["moments"].tobytes() == host["moments"].tobytes()
    assert not np.array_equal(host["place"], base) and any(w[1] for w in want["contacts", use_keep, use_boxes])
    assert np.array_equal(d_world.download(), world)
    for h in list(dsts.values()) + [labels, medium, d_world]:
        h.close()


def test_trace_paths_in_host_form_returns_what_it_did_not_write(built):
    """the paths are the part that goes up and comes back: lengths and routes are the model's, and every entry beyond a
    route's length still holds what the caller left there"""
    import cpuvoxelraycaster_amd as vrc
    capi = vrc.capi
    S, SENTINEL = 16, 0xA5A5A5A5
    vol = np.zeros((S, S, S), np.uint8)
    vol[1:15, 4, 3] = 1                                           # a corridor with a bend, seeded at one end
    vol[14, 4:12, 3] = 1
    vol[2, 9, 9] = 1                                              # solid, but joined to nothing: unreachable
    seeds = np.zeros_like(vol)
    seeds[1, 4, 3] = 1
    T = travel_model.field(vol, seeds, 6)
    starts = np.array([[14, 11, 3], [2, 9, 9], [5, 4, 3]], np.uint32)
    model = [travel_model.trace(T, tuple(int(v) for v in s), 6) for s in starts]
    assert [m[0] for m in model] == [20, travel_model.NONE, 4]
    capacity = 24                                                 # more than the longest route's 21 voxels
    medium, d_seeds = volume_of(vol), volume_of(seeds)
    field = medium.travelField(d_seeds, 6)
    lengths = np.full(3, SENTINEL, np.uint32)
    paths = np.full((3, capacity, 3), SENTINEL, np.uint32)
    capi.check(capi.load().vrc_travel_trace_paths(field._h, 3, capi.ptr(starts), capacity, capi.ptr(paths), capi.ptr(lengths), capi.VRC_MEM_HOST, None))
    for i, (length, route) in enumerate(model):
        assert int(lengths[i]) == length, i
        assert np.array_equal(paths[i, :len(route)], route), i
        assert (paths[i, len(route):] == SENTINEL).all(), i
    assert [len(m[1]) for m in model] == [21, 0, 5]
    for h in (field, medium, d_seeds):
        h.close()


def test_a_call_with_a_block_of_its_own_keeps_nothing_between_calls(built):
    """host-form contacts on labels of 7 pieces, then on labels of 20: each call lays out a block for its own count"""
    vol, offsets, maps, boxes, keep, base, world, want = piece_case()
    d_world = volume_of(world)
    medium = volume_of(vol)
    labels = medium.labelComponents(6)
    got = labels.contacts(affine_records(maps), d_world, boxes, keep)
    assert [contact_model.record_tuple(r) for r in got] == want["contacts", True, True]
    labels.close()
    medium.close()

    more = scattered_blocks(extra=13)
    ids, records = components_model.label(more, 6)
    assert len(records) == 20
    rng = np.random.default_rng(4701)
    offsets = rng.integers(-3, 4, (20, 3)).astype(np.int32)
    maps, boxes = rigid_model.translation_maps(offsets), rigid_model.moved_boxes(records, offsets, 16)
    keep = (np.arange(20) % 4 != 2).astype(np.uint8)
    medium = volume_of(more)
    labels = medium.labelComponents(6)
    assert labels.count == 20
    got = labels.contacts(affine_records(maps), d_world, boxes, keep)
    assert [contact_model.record_tuple(r) for r in got] == contact_model.contacts(ids, maps, boxes, world, keep)
    for h in (labels, medium, d_world):
        h.close()


def test_contacts_in_device_memory_behind_an_edit_of_the_world_on_another_stream(built):
    """a device-memory fill of the world on one stream, then contactsDevice against it on another with no synchronisation:
    the records are those of the edited world -- once at 16^3, and once behind edits that take long enough to lose a race
    against, a 512^3 world filled and cleared sixteen times over"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    vol, offsets, maps, boxes, keep, base, world, _ = piece_case()
    ids, _ = components_model.label(vol, 6)
    medium = volume_of(vol)
    labels = medium.labelComponents(6)
    count = labels.count
    box = np.array([[0, 5, 0, 16, 9, 16]], np.uint32)
    edited = world.copy()
    edited[0:16, 5:9, 0:16] = 1
    want = contact_model.contacts(ids, maps, boxes, edited, keep)
    assert want != contact_model.contacts(ids, maps, boxes, world, keep)
    # the same pieces, unmoved, inside a 512^3 world that ends full: every posed voxel overlaps
    big, B = vrc.VoxelVolume(9), 512
    identity = rigid_model.translation_maps(np.zeros((count, 3), np.int32))
    voxels = np.bincount(ids[ids != components_model.NO_COMPONENT].astype(np.int64), minlength=count)

    d_world = volume_of(world)
    t_maps, t_identity = device_bytes(affine_records(maps)), device_bytes(affine_records(identity))
    t_boxes, t_keep, t_box = device_bytes(boxes), device_bytes(keep), device_bytes(box)
    t_whole = device_bytes(np.array([[0, 0, 0, B, B, B]], np.uint32))
    t_out = torch.full((count * 128,), 0x5A, dtype=torch.uint8).cuda()
    t_big_out = torch.full((count * 128,), 0x5A, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with Stream() as first, Stream() as second:
        d_world.fillBoxesDevice(1, t_box.data_ptr(), True, first)
        labels.contactsDevice(t_maps.data_ptr(), d_world, t_out.data_ptr(), t_boxes.data_ptr(), t_keep.data_ptr(), second)
        for round_ in range(16):
            big.fillBoxesDevice(1, t_whole.data_ptr(), round_ % 2 == 1, first)
        labels.contactsDevice(t_identity.data_ptr(), big, t_big_out.data_ptr(), None, None, second)
    got = t_out.cpu().numpy().view(vrc.capi.CONTACT_DTYPE)
    assert [contact_model.record_tuple(r) for r in got] == want
    got = t_big_out.cpu().numpy().view(vrc.capi.CONTACT_DTYPE)
    assert got["posed"].tolist() == voxels.tolist() and got["overlap"].tolist() == voxels.tolist()
    assert np.array_equal(d_world.download(), edited)
    for h in (labels, medium, d_world, big):
        h.close()


# ---- the windowed lists: the prologue of the emit pass (vrc_list.h: list_window) and the wrapper's paged fetch ------------
#
# The list tests (test_gpu_volume_surface / _voxels / _rects: test_windows) put window edges inside a lane, on a workgroup
# edge and at first >= T, on 64^3 and 32^3 fields at 50 %; none of them has capacity 0 with a buffer, first = T + 1, a
# capacity that overflows first + capacity, or both cuts inside lanes of different workgroups, and none uses these fields.

SENTINEL = 0x5A5A5A5A
LIST_KINDS = ("faces", "voxels_xyz", "voxels_neighbours", "rects")


@functools.lru_cache(maxsize=None)
def list_case(kind):
    """(the field, the model's full list, records per lane of the emit pass), computed once and never written again"""
    if kind == "rects":
        vol = random_volume(4800, 4, 0.37)                      # 16^3: 6 * 256 lanes, 6 workgroups
        want = rect_model.rects(vol, True)
        lanes = np.bincount(rect_cases.lane_of(want, 16), minlength=rect_cases.lanes_of(4))
    else:
        vol = random_volume(4801, 5, 0.37)                      # 32^3: 1024 words, 4 workgroups
        if kind == "faces":
            want = surface_model.faces(vol, True)
            lanes = surface_model.word_direction_counts(want, 32).sum(axis=1)
        else:
            want = voxels_model.voxels_dense(vol, voxels_model.SURFACE, None, True, kind == "voxels_neighbours")
            lanes = np.bincount(surface_model.key_of(want[:, :3], 32) >> 5, minlength=1024)
    assert lanes.sum() == len(want)
    for a in (vol, want, lanes):
        a.setflags(write=False)
    return vol, want, lanes


@pytest.mark.parametrize("kind", LIST_KINDS)
def test_list_windows_through_the_shared_prologue(built, kind):
    """every window into device memory pre-filled with a sentinel: the records are the slice of the model's list, and
    everything beyond min(capacity, T - first) records is untouched"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    capi = vrc.capi
    vol, want, lanes = list_case(kind)
    T, per = want.shape
    start = np.concatenate([[0], np.cumsum(lanes)])
    groups = len(lanes) // 256
    busy = np.flatnonzero(lanes >= 3)
    a, b = int(busy[busy // 256 == 1][0]), int(busy[busy // 256 == groups - 2][-1])
    first_cut, last_cut = int(start[a]) + 1, int(start[b]) + 2   # both inside a lane's run of records, workgroups apart
    assert start[a] < first_cut < start[a + 1] and start[b] < last_cut < start[b + 1] and a // 256 < b // 256
    windows = [(first_cut, last_cut - first_cut), (first_cut, 1), (5, 0), (T, 4), (T + 1, 4), (3, 2 ** 64 - 1)]
    assert first_cut + 1 < start[a + 1]                          # the second window lies wholly inside lane a
    volume = volume_of(vol)
    fetch = {"faces": lambda *w: volume.extractSurfaceDevice(capi.VRC_SURFACE_FACES, *w),
             "voxels_xyz": lambda *w: volume.extractVoxelsDevice(capi.VRC_VOXELS_SURFACE, capi.VRC_VOXELS_XYZ, *w),
             "voxels_neighbours": lambda *w: volume.extractVoxelsDevice(capi.VRC_VOXELS_SURFACE, capi.VRC_VOXELS_NEIGHBOURS, *w),
             "rects": lambda *w: volume.extractRectsDevice(capi.VRC_SURFACE_FACES, *w)}[kind]
    for first, capacity in windows:
        n = max(0, min(capacity, T - first))
        dev = torch.full((n + 4, per), SENTINEL, dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        fetch(first, capacity, dev.data_ptr(), total.data_ptr())
        torch.cuda.synchronize()
        got = dev.cpu().numpy().view(np.uint32)
        assert int(total.item()) == T, (first, capacity)
        assert np.array_equal(got[:n], want[first:first + n]), (first, capacity)
        assert (got[n:] == SENTINEL).all(), (first, capacity)
    volume.close()


def test_paged_fetch_is_the_same_at_any_window(built, monkeypatch):
    """the six host-form list calls with SURFACE_WINDOW = 7 against the default window, whole and from 5 for 23; beyond the
    total they are empty arrays of the right shape and dtype"""
    import cpuvoxelraycaster_amd as vrc
    volume = volume_of(random_volume(4802, 4, 0.37))
    calls = {"surfaceFaces": (lambda **w: volume.surfaceFaces(**w), (0, 4), np.uint32),
             "surfaceTriangles": (lambda **w: volume.surfaceTriangles(**w), (0, 9), np.int32),
             "voxels": (lambda **w: volume.voxels(**w), (0, 3), np.uint32),
             "voxels(neighbours)": (lambda **w: volume.voxels(neighbours=True, **w), (0, 4), np.uint32),
             "surfaceRects": (lambda **w: volume.surfaceRects(**w), (0, 4), np.uint32),
             "rectTriangles": (lambda **w: volume.rectTriangles(**w), (0, 9), np.int32)}
    whole = {name: call() for name, (call, _, _) in calls.items()}
    part = {name: call(first=5, capacity=23) for name, (call, _, _) in calls.items()}
    assert vrc.VoxelVolume.SURFACE_WINDOW > 7
    monkeypatch.setattr(vrc.VoxelVolume, "SURFACE_WINDOW", 7)
    for name, (call, empty, dtype) in calls.items():
        rows = empty[1] // 9 + 1                                  # two triangles a record
        assert len(whole[name]) > 7 * rows * 3, name              # several windows
        assert np.array_equal(whole[name][5 * rows:28 * rows], part[name]) and len(part[name]) == 23 * rows, name
        assert np.array_equal(call(), whole[name]), name
        assert np.array_equal(call(first=5, capacity=23), part[name]), name
        for first in (len(whole[name]) // rows, len(whole[name]) // rows + 1):
            for capacity in (None, 4):
                got = call(first=first, capacity=capacity)
                assert got.shape == empty and got.dtype == dtype, (name, first, capacity)
    volume.close()


def test_fetch_of_a_known_count(built):
    """components, moments, pieceSites and records from 0, from 3 for 2, from count and from count + 1"""
    vol = scattered_blocks()
    sites = np.array([[2, 2, 2], [13, 13, 13]], np.int32)          # no block straddles the two cells
    ids, rec, piece_sites = fracture_model.label(vol, sites, 6)
    assert len(rec) == 7 and len(set(piece_sites.tolist())) == 2
    moments = rigid_model.moments(ids, 7)
    medium, empty = volume_of(vol), volume_of(np.zeros_like(vol))
    labels, delta = medium.fracture(sites, 6), empty.diff(medium)
    records, _ = delta_model.diff(delta_model.words_of(np.zeros_like(vol)), delta_model.words_of(vol), 4)
    assert labels.count == 7 and delta.count == len(records) >= 5
    for count, first, capacity in [(7, 0, None), (7, 3, 2), (7, 7, None), (7, 7, 3), (7, 8, None), (7, 8, 3)]:
        k = slice(first, count if capacity is None else min(count, first + capacity))
        got = labels.components(first, capacity)
        assert got.dtype == labels.components().dtype and got.shape == (max(0, k.stop - first),)
        for field in ("first", "lo", "hi", "voxels"):
            assert np.array_equal(got[field], rec[k][field]), (first, capacity, field)
        assert [rigid_model.moments_tuple(r) for r in labels.moments(first, capacity)] == moments[k], (first, capacity)
        got = labels.pieceSites(first, capacity)
        assert got.dtype == np.uint32 and np.array_equal(got, piece_sites[k]), (first, capacity)
    n = delta.count
    for first, capacity in [(0, None), (3, 2), (n, None), (n, 3), (n + 1, None), (n + 1, 3)]:
        got = delta.records(first, capacity)
        want = records[first:n if capacity is None else first + capacity]
        assert got.dtype == delta.records().dtype and got.tobytes() == want.tobytes(), (first, capacity)
    for h in (labels, delta, medium, empty):
        h.close()
