"""Volume deltas on the device (include/vrc.h: vrc_delta_diff, vrc_delta_*) against the numpy model of delta_model.py:
records, stats and every download are compared bit for bit.  The diff's workgroup takes 256 words (csrc/vrc_delta.hip), so
256^3 with its 2048 slots is the first size at which the slot scan takes a second step."""
import ctypes as C

import numpy as np
import pytest

import delta_model as model
import distance_model
from volume_support import Stream, committed, expected_nodes, same, terrain_volume, volume_of

pytestmark = pytest.mark.gpu


def words_on_device(volume):
    return model.words_of(volume.download())


def check_delta(delta, wa, wb, depth, what):
    """records, stats, count and bytes of a delta of the word arrays wa -> wb"""
    records, stats = model.diff(wa, wb, depth)
    assert delta.count == len(records) and delta.bytes() == 8 * len(records), (what, delta.count, len(records))
    assert model.stats_tuple(delta.stats) == model.stats_tuple(stats), (what, model.stats_tuple(delta.stats), model.stats_tuple(stats))
    got = delta.records()
    bad = np.flatnonzero((got["word"] != records["word"]) | (got["bits"] != records["bits"]))
    assert not len(bad), (what, len(bad), got[bad[:3]].tolist(), records[bad[:3]].tolist())
    return records


def check_pair(before, after, wa, wb, depth, what):
    """diff(before, after) against the model; applied to a clone of before it gives after, applied again before"""
    delta = before.diff(after)
    check_delta(delta, wa, wb, depth, what)
    probe = before.clone()
    probe.applyDelta(delta)
    assert np.array_equal(words_on_device(probe), wb), (what, "apply")
    probe.applyDelta(delta)
    assert np.array_equal(words_on_device(probe), wa), (what, "apply twice")
    probe.close()
    assert np.array_equal(words_on_device(before), wa) and np.array_equal(words_on_device(after), wb), (what, "the volumes are only read")
    delta.close()


# ---- 1. random pairs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_random_pairs(built, depth):
    S = 1 << depth
    rng = np.random.default_rng(100 + depth)
    for density in (0.02, 0.5, 0.98):
        a = (rng.random((S, S, S)) < density).astype(np.uint8)
        b = a ^ (rng.random((S, S, S)) < 0.01).astype(np.uint8)
        if depth == 2:
            b[tuple(rng.integers(0, S, 3))] ^= 1            # 64 voxels: 1 % may flip none
        before, after = volume_of(a, depth), volume_of(b, depth)
        check_pair(before, after, model.words_of(a), model.words_of(b), depth, (depth, density))
        if density == 0.5:
            twin = before.clone()
            check_pair(before, twin, model.words_of(a), model.words_of(a), depth, (depth, "a against its clone"))
            twin.close()
        before.close()
        after.close()
    empty, other, full = np.zeros((S, S, S), np.uint8), np.zeros((S, S, S), np.uint8), np.ones((S, S, S), np.uint8)
    for x, y, what in [(empty, other, "empty / empty"), (empty, full, "empty / full"), (full, empty, "full / empty")]:
        before, after = volume_of(x, depth), volume_of(y, depth)
        check_pair(before, after, model.words_of(x), model.words_of(y), depth, (depth, what))
        before.close()
        after.close()


# ---- 2. 4^3 by hand: a word holds two brick rows --------------------------------------------------------------------

def test_depth_2_by_hand(built):
    import cpuvoxelraycaster_amd as vrc
    first, second = (1, 3, 2), (2, 1, 3)                      # key 27 = word 0 bit 27 (row cy = 1); key 46 = word 1 bit 14 (row cy = 0)
    cases = [([first], [(0, 1 << 27)], (1, 1, first, (2, 4, 3), (0, 0))),
             ([second], [(1, 1 << 14)], (1, 1, second, (3, 2, 4), (0, 0))),
             ([first, second], [(0, 1 << 27), (1, 1 << 14)], (2, 2, (1, 1, 2), (3, 4, 4), (0, 0))),
             ([(0, 0, 0), (0, 2, 1)], [(0, (1 << 0) | (1 << 20))], (1, 2, (0, 0, 0), (1, 3, 2), (0, 0))),      # both rows of word 0
             ([(3, 1, 3), (3, 3, 0)], [(1, (1 << 15) | (1 << 19))], (1, 2, (3, 1, 0), (4, 4, 4), (0, 0)))]
    for voxels, records, stats in cases:
        before, after = vrc.VoxelVolume(2), vrc.VoxelVolume(2)
        before.fillBoxes([[0, 0, 0, 4, 2, 4]])
        after.fillBoxes([[0, 0, 0, 4, 2, 4]])
        solid = np.array([v[1] >= 2 for v in voxels])         # outside the slab: set; inside it: cleared
        if solid.any():
            after.setVoxels(np.array(voxels)[solid], True)
        if (~solid).any():
            after.setVoxels(np.array(voxels)[~solid], False)
        delta = before.diff(after)
        assert delta.records().tolist() == records, voxels
        assert model.stats_tuple(delta.stats) == stats, (voxels, model.stats_tuple(delta.stats))
        for volume in (before, after):
            volume.close()
        delta.close()


# ---- 3. 256^3: the slot scan's second step --------------------------------------------------------------------------

def voxel_of_bit(word, bit, depth):
    n = 1 << (depth - 1)
    key = 32 * word + bit
    B = key >> 3
    return (2 * (B // (n * n)) + (key & 1), 2 * ((B // n) % n) + ((key >> 1) & 1), 2 * (B % n) + ((key >> 2) & 1))


@pytest.fixture(scope="module")
def large(built):
    import cpuvoxelraycaster_amd as vrc
    S = 256
    empty, full = vrc.VoxelVolume(8), vrc.VoxelVolume(8)
    full.fillBoxes([[0, 0, 0, S, S, S]])
    yield empty, full, np.zeros(S ** 3 // 32, np.uint32), np.full(S ** 3 // 32, 0xFFFFFFFF, np.uint32)
    empty.close()
    full.close()


def test_every_word_differs_at_256(large):
    empty, full, w_empty, w_full = large
    delta = empty.diff(full)
    assert delta.count == 524288 == 2048 * 256                # the largest slot values: 2048 slots of 256 records each
    check_delta(delta, w_empty, w_full, 8, "empty / full at 256^3")
    probe = empty.clone()
    probe.applyDelta(delta)
    assert probe.solidCount() == 256 ** 3
    probe.applyDelta(delta)
    assert probe.solidCount() == 0
    probe.close()
    delta.close()


def test_single_voxels_by_word_index_at_256(large):
    empty, _, w_empty, _ = large
    n_words = len(w_empty)
    # word 0, the last word, the last word of workgroup 0 and the first of workgroup 1, either side of the slot 1023 / 1024 boundary
    places = [(0, 0), (n_words - 1, 31), (255, 9), (256, 22), (1023 * 256 + 255, 31), (1024 * 256, 0), (1024 * 256 - 256, 5), (1025 * 256 - 1, 17)]
    after = empty.clone()
    after.setVoxels([voxel_of_bit(w, b, 8) for w, b in places])
    wb = w_empty.copy()
    for w, b in places:
        wb[w] |= 1 << b
    assert np.array_equal(words_on_device(after), wb)
    delta = empty.diff(after)
    assert sorted(delta.records().tolist()) == delta.records().tolist() == sorted((w, 1 << b) for w, b in places)
    check_delta(delta, w_empty, wb, 8, "single voxels")
    probe = empty.clone()
    probe.applyDelta(delta)
    assert np.array_equal(words_on_device(probe), wb)
    for volume in (probe, after):
        volume.close()
    delta.close()


def test_sphere_dug_at_256(large):
    _, full, _, w_full = large
    S = 256
    after = full.clone()
    after.fillSpheres([(128, 120, 131, 20)], False)
    dense = np.ones((S, S, S), np.uint8)
    x, y, z = np.ogrid[:S, :S, :S]
    dense[(x - 128) ** 2 + (y - 120) ** 2 + (z - 131) ** 2 <= 400] = 0
    wb = model.words_of(dense)
    delta = full.diff(after)
    check_delta(delta, w_full, wb, 8, "sphere")
    assert tuple(delta.stats.lo) == (108, 100, 111) and tuple(delta.stats.hi) == (149, 141, 152)
    probe = after.clone()
    probe.applyDelta(delta)                                   # undo: after -> before
    assert probe.solidCount() == S ** 3
    for volume in (probe, after):
        volume.close()
    delta.close()


# ---- 4. windows -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair_32(built):
    rng = np.random.default_rng(7)
    a = (rng.random((32, 32, 32)) < 0.5).astype(np.uint8)
    b = a ^ (rng.random((32, 32, 32)) < 0.01).astype(np.uint8)
    before, after = volume_of(a, 5), volume_of(b, 5)
    delta = before.diff(after)
    yield before, after, model.words_of(a), model.words_of(b), delta
    for thing in (delta, before, after):
        thing.close()


def test_record_windows(pair_32):
    import torch
    from cpuvoxelraycaster_amd import capi
    _, _, wa, wb, delta = pair_32
    records, _ = model.diff(wa, wb, 5)
    count = len(records)
    assert count > 20
    L = capi.load()
    for first, capacity in [(0, count), (0, 0), (3, 5), (count - 1, 10), (count, 4), (count + 7, 1)]:
        want = records[first:first + capacity]
        host = np.full(2 * (capacity + 4), 0xABABABAB, np.uint32)             # two records of canary on either side
        capi.check(L.vrc_delta_records(delta._h, first, capacity, capi.ptr(host[4:]), capi.VRC_MEM_HOST, None))
        dev = torch.full((2 * (capacity + 4),), 0x2B2B2B2B, dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        with Stream() as stream:
            delta.recordsDevice(first, capacity, dev.data_ptr() + 16, stream)
        got = dev.cpu().numpy().view(np.uint32)
        for buf, canary in ((host, 0xABABABAB), (got, 0x2B2B2B2B)):
            assert buf[4:4 + 2 * len(want)].tobytes() == want.tobytes(), (first, capacity)
            assert (buf[:4] == canary).all() and (buf[4 + 2 * len(want):] == canary).all(), (first, capacity)
        assert np.array_equal(delta.records(first, capacity), want)
    assert L.vrc_delta_records(delta._h, 0, 0, None, capi.VRC_MEM_HOST, None) == 0


# ---- 5. create ------------------------------------------------------------------------------------------------------

def test_create_round_trip(pair_32):
    import torch
    import cpuvoxelraycaster_amd as vrc
    before, _, wa, wb, delta = pair_32
    records = delta.records()
    dev = torch.from_numpy(records.view(np.uint32).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    for made in (vrc.VoxelDelta.fromRecords(5, records), before.deltaFromRecords(records.view(np.uint32).reshape(-1, 2)),
                 vrc.VoxelDelta.fromRecordsDevice(5, len(records), dev.data_ptr()), before.deltaFromRecordsDevice(len(records), dev.data_ptr())):
        check_delta(made, wa, wb, 5, "from records")
        stats = capi_stats(made)
        assert model.stats_tuple(stats) == model.stats_tuple(delta.stats)
        probe = before.clone()
        probe.applyDelta(made)
        assert np.array_equal(words_on_device(probe), wb)
        probe.close()
        made.close()
    nothing = vrc.VoxelDelta.fromRecords(5, np.zeros(0, vrc.DELTA_RECORD_DTYPE))
    assert nothing.count == 0 and nothing.bytes() == 0 and model.stats_tuple(nothing.stats) == (0, 0, (0, 0, 0), (0, 0, 0), (0, 0))
    assert len(nothing.records()) == 0
    before.applyDelta(nothing)
    assert np.array_equal(words_on_device(before), wa)
    nothing.close()
    # 4^3, both words, the last word's last bit
    small = vrc.VoxelDelta.fromRecords(2, [(0, 1), (1, 0x80000000)])
    assert model.stats_tuple(small.stats) == (2, 2, (0, 0, 0), (4, 4, 4), (0, 0))
    small.close()


def capi_stats(delta):
    from cpuvoxelraycaster_amd import capi
    stats = capi.DeltaStats()
    capi.check(capi.load().vrc_delta_get_stats(delta._h, C.byref(stats)))
    return stats


def test_create_refuses_a_bad_list(pair_32):
    import torch
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    delta = pair_32[4]
    good = delta.records()
    n_words = 32 ** 3 // 32
    L = capi.load()

    def refused(records, index, depth=5):
        records = np.ascontiguousarray(records)
        dev = torch.from_numpy(records.view(np.uint32).view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        for mem, p in ((capi.VRC_MEM_HOST, capi.ptr(records)), (capi.VRC_MEM_DEVICE, dev.data_ptr())):
            out, stats = C.c_void_p(0x55), capi.DeltaStats()
            stats.words = 7
            assert L.vrc_delta_create(depth, 0, len(records), p, mem, C.byref(out), C.byref(stats)) == -1
            text = L.vrc_last_error().decode()
            assert text.startswith("vrc_delta_create: record %d" % index) and not text[len("vrc_delta_create: record %d" % index)].isdigit(), (index, text)
            assert out.value == 0x55 and stats.words == 7
        with pytest.raises(vrc.VrcError):
            vrc.VoxelDelta.fromRecords(depth, records)

    swapped = good.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    refused(swapped, 11)
    duplicate = good.copy()
    duplicate[5]["word"] = duplicate[4]["word"]
    refused(duplicate, 5)
    beyond = good.copy()
    beyond[-1]["word"] = n_words
    refused(beyond, len(good) - 1)
    zero = good.copy()
    zero[0]["bits"] = 0
    refused(zero, 0)
    several = good.copy()
    several[17]["bits"] = 0
    several[[8, 9]] = several[[9, 8]]
    several[-1]["word"] = 0xFFFFFFFF
    refused(several, 9)
    # more records than the volume has words: the rule breaks within the first n_words + 1
    refused(np.array([(0, 1), (1, 1), (2, 1)], capi.DELTA_RECORD_DTYPE), 2, depth=2)
    refused(np.array([(0, 1), (0, 1), (0, 1), (0, 1), (0, 1)], capi.DELTA_RECORD_DTYPE), 1, depth=2)


# ---- 6. ordering ----------------------------------------------------------------------------------------------------

def test_ordering_on_a_stream(pair_32):
    import torch
    before, after, wa, wb, delta = pair_32
    rng = np.random.default_rng(11)
    extra = rng.integers(0, 32, (5000, 3)).astype(np.uint32)
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    dense = model.dense_of(wa, 5)
    dense[tuple(extra.astype(np.int64).T)] = 1
    w_edit = model.words_of(dense)
    torch.cuda.synchronize()
    # a device-memory edit, then the apply on the same stream, then commit: nothing between them
    volume = before.clone()
    with Stream() as stream:
        volume.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
        volume.applyDelta(delta, stream)
        nodes = committed(volume)
    records, _ = model.diff(wa, wb, 5)
    state = model.dense_of(model.apply(w_edit, records), 5)
    assert same(nodes, expected_nodes(state, 5))
    assert np.array_equal(volume.download(), state)
    volume.close()
    # a diff right behind a device-memory edit sees it, on either side
    for side in (0, 1):
        volume = before.clone()
        with Stream() as stream:
            volume.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
            seen = volume.diff(after) if side == 0 else after.diff(volume)
        check_delta(seen, *((w_edit, wb) if side == 0 else (wb, w_edit)), 5, ("behind a device edit", side))
        seen.close()
        volume.close()


# ---- 7. history -----------------------------------------------------------------------------------------------------

def numpy_sphere(vol, cx, cy, cz, r, value):
    S = vol.shape[0]
    x, y, z = np.ogrid[:S, :S, :S]
    vol[(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r] = value


def test_history_at_64(built, heights):
    import cpuvoxelraycaster_amd as vrc
    depth = 6
    states = [terrain_volume(heights, depth)]
    volume = volume_of(states[0], depth)
    history = vrc.VoxelHistory(volume)

    def holds(k, what):
        assert np.array_equal(volume.download(), states[k]), what

    states.append(states[-1].copy())
    numpy_sphere(states[-1], 30, 36, 33, 8, 0)
    volume.fillSpheres([(30, 36, 33, 8)], False)
    dig = history.record()
    states.append(states[-1].copy())
    states[-1][10:20, 10:20, 11:21] = 1                       # in the air: the terrain starts at y = S/2 + 1
    volume.fillBoxes([[10, 10, 11, 20, 20, 21]])
    box = history.record()
    states.append(distance_model.dilate(states[-1], 2).astype(np.uint8))
    volume.dilate(2)
    grown = history.record()
    assert history.record() is None and (history.undoCount, history.redoCount) == (3, 0)
    for k, delta in enumerate((dig, box, grown)):
        check_delta(delta, model.words_of(states[k]), model.words_of(states[k + 1]), depth, ("step", k))
    assert tuple(box.stats.lo) == (10, 10, 11) and tuple(box.stats.hi) == (20, 20, 21) and box.stats.voxels == 1000
    assert history.bytes() == 8 * (dig.count + box.count + grown.count)
    holds(3, "three edits")
    assert history.undo() is grown
    holds(2, "undo 1")
    assert history.undo() is box
    holds(1, "undo 2")
    assert history.undo() is dig
    holds(0, "undo 3")
    assert history.undo() is None and (history.undoCount, history.redoCount) == (0, 3)
    assert history.redo() is dig
    holds(1, "redo 1")
    assert history.redo() is box
    holds(2, "redo 2")
    # a new edit: the redo stack goes
    branch = states[2].copy()
    numpy_sphere(branch, 40, 30, 20, 5, 1)
    volume.fillSpheres([(40, 30, 20, 5)], True)
    ball = history.record()
    assert ball is not None and (history.undoCount, history.redoCount) == (3, 0) and history.redo() is None
    assert grown._h is None                                   # dropped with the redo stack, closed
    assert np.array_equal(volume.download(), branch)
    assert history.undo() is ball
    holds(2, "undo of the branch")
    assert history.record() is None                           # the shadow followed every step
    history.close()
    volume.close()


def test_history_drops_the_oldest_beyond_max_bytes(built):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(6)
    history = vrc.VoxelHistory(volume, max_bytes=8 * 40)
    steps = []
    for k in range(4):
        volume.fillBoxes([[8 * k, 0, 0, 8 * k + 2, 4, 128]])     # two brick rows along z: 16 words each
        steps.append(history.record())
        assert steps[-1].count == 16
    assert history.undoCount == 2 and history.bytes() == 8 * 32 and steps[0]._h is None and steps[1]._h is None
    assert history.undo() is steps[3] and history.undo() is steps[2] and history.undo() is None
    assert volume.solidCount() == 2 * 2 * 4 * 64
    volume.fillBoxes([[0, 0, 0, 64, 64, 64]])                 # one step above the limit alone: kept, everything older dropped
    big = history.record()
    assert big.bytes() > 8 * 40 and history.undoCount == 1 and history.redoCount == 0
    history.close()
    volume.close()


def test_dig_at_a_hit_and_undo_at_128(built, heights):
    import cpuvoxelraycaster_amd as vrc
    depth = 7
    scene = vrc.LSVO.fromTerrain(heights, depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    first_commit = committed(volume)
    history = vrc.VoxelHistory(volume)
    cam = vrc.reference_camera(depth, pitch=-0.5)
    org = (np.array(tuple(cam.position), np.float32) / np.float32(1 << depth) + np.float32(1.0)).astype(np.float32)
    rot = np.array(tuple(cam.rot), np.float32)
    hit = scene.castRay(org, np.array([rot[2], rot[5], rot[8]], np.float32))
    assert (hit["hit"] & 0xff) == 1
    volume.fillSpheresAtHits(np.array([hit]), 4, False)
    step = history.record()
    voxel, _ = vrc.hit_to_voxel(depth, hit)
    assert step is not None and all(lo <= c < hi for lo, c, hi in zip(step.stats.lo, voxel, step.stats.hi))
    assert not same(committed(volume), first_commit)
    assert history.undo() is step
    assert same(committed(volume), first_commit)
    history.close()
    volume.close()
    scene.close()


# ---- 8. no growth, 9. mismatches ------------------------------------------------------------------------------------

def test_twenty_rounds_leave_no_scratch(built):
    import cpuvoxelraycaster_amd as vrc
    before, after = vrc.VoxelVolume(6), vrc.VoxelVolume(6)
    before.fillBoxes([[0, 0, 0, 64, 20, 64]])
    after.fillBoxes([[0, 0, 0, 64, 20, 64]])
    after.fillSpheres([(30, 20, 30, 6)], False)
    at_start = (before.editScratchBytes(), after.editScratchBytes())
    want = None
    for _ in range(20):
        delta = before.diff(after)
        records = delta.records()
        want = records if want is None else want
        assert records.tobytes() == want.tobytes() and len(records)
        after.applyDelta(delta)
        after.applyDelta(delta)
        delta.close()
        assert (before.editScratchBytes(), after.editScratchBytes()) == at_start
    before.close()
    after.close()


def test_apply_refuses_another_depth(pair_32):
    import cpuvoxelraycaster_amd as vrc
    delta = pair_32[4]
    for depth in (4, 6):
        other = vrc.VoxelVolume(depth)
        with pytest.raises(vrc.VrcError, match="vrc_delta_apply: delta of depth 5, volume of depth %d" % depth):
            other.applyDelta(delta)
        assert other.solidCount() == 0
        other.close()
    made = vrc.VoxelDelta.fromRecords(4, [(3, 5)])
    with pytest.raises(vrc.VrcError, match="vrc_delta_diff: volumes of depths"):
        pair_32[0].diff(vrc.VoxelVolume(4))
    with pytest.raises(vrc.VrcError):
        pair_32[0].applyDelta(made)
    made.close()
