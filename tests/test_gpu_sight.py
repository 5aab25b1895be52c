"""Line of sight and visible sets on the GPU (vrc_sight_segments, vrc_sight_field; VoxelDistance.sight / sightDevice /
visibleFrom, VoxelVolume.lineOfSight / visibleFrom, smoothPath).  Every comparison is byte-exact against tests/sight_model.py,
which tests/test_sight_host.py holds to the geometry; the device's own field is first held to tests/distance_model.py or
tests/travel_model.py, so that model and device walk over the same values.  The cases come from tests/sight_cases.py."""
import ctypes as C

import numpy as np
import pytest

import distance_model
import sight_cases as cases
import sight_model as model
import travel_model
from volume_support import Stream, device_words, volume_of

pytestmark = pytest.mark.gpu

NONE = model.NONE


def euclidean(vol, to_empty=False, outside=False):
    """(VoxelDistance, its values by the numpy model), the two held equal"""
    volume = volume_of(vol)
    field = volume.distanceField(to_empty, outside)
    volume.close()
    D = distance_model.field(vol, to_empty, outside)
    assert np.array_equal(field.download(), D)
    return field, D


def device_sight(field, segments, lo, hi, touch, plain, guard=0):
    """the records through device memory on a stream of the test's own, with `guard` records behind them that must stay"""
    import torch
    from cpuvoxelraycaster_amd import capi
    n = len(segments)
    d_segments = device_words(segments)
    d_out = torch.full(((n + guard) * 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                      # the test's stream does not wait for the NULL stream that filled them
    with Stream() as stream:
        field.sightDevice(n, d_segments.data_ptr(), d_out.data_ptr(), lo, hi, touch, plain, stream)
    raw = d_out.cpu().numpy().view(np.uint32)
    assert (raw[n * 8:] == 0x5A5A5A5A).all()
    return raw[:n * 8].view(capi.SIGHT_DTYPE)


def every_way(field, segments, lo, hi, touch, want):
    """host and device memory, the stride (where the field allows it) and VRC_SIGHT_PLAIN: all the bytes of `want`"""
    a, b = segments[:, :3], segments[:, 3:]
    for plain in (False, True):
        got = field.sight(a, b, lo, hi, touch, plain)
        assert got.tobytes() == want.tobytes(), (lo, hi, touch, plain, [(i, got[i], want[i]) for i in np.flatnonzero(got != want)[:3]])
        assert device_sight(field, segments, lo, hi, touch, plain).tobytes() == want.tobytes(), (lo, hi, touch, plain)


# ---- 1. 8^3 ---------------------------------------------------------------------------------------------------------

def test_every_segment_from_four_starts_at_8(built):
    S = 8
    vol = cases.random_solid(S, 0.1, 101)
    field, D = euclidean(vol)
    empty = np.argwhere(vol == 0)
    starts = [tuple(empty[0]), tuple(empty[len(empty) // 3]), tuple(empty[-1]), tuple(np.argwhere(vol)[0])]
    segments = cases.starts_to_all(S, starts)
    for touch in (False, True):
        want = model.sight(D, S, segments, 1, NONE, touch)
        assert {int(s) for s in want["status"]} == {model.CLEAR, model.BLOCKED}
        every_way(field, segments, 1, NONE, touch, want)
    field.close()


# ---- 2. ties ---------------------------------------------------------------------------------------------------------

def test_ties_at_16(built):
    S = 16
    segments = cases.tie_segments(S)
    vol = cases.random_solid(S, 0.02, 102)
    vol[S // 2, S // 2, S // 2] = 0
    field, D = euclidean(vol)
    for touch in (False, True):
        every_way(field, segments, 1, NONE, touch, model.sight(D, S, segments, 1, NONE, touch))
    field.close()


def test_two_solids_that_touch_diagonally(built):
    from cpuvoxelraycaster_amd import capi
    for solid, a, b, thin, touch in cases.diagonal_pair_cases(16):
        field, D = euclidean(solid)
        for mode, want in ((False, thin), (True, touch)):
            assert model.segment(D, 16, a, b, 1, NONE, mode) == want
            for plain in (False, True):
                rec = field.sight(a, b, 1, NONE, mode, plain)[0]
                assert (int(rec["status"]), tuple(int(v) for v in rec["at"]), tuple(int(v) for v in rec["before"])) == want
        assert want[0] == capi.VRC_SIGHT_BLOCKED
        field.close()


# ---- 3. stride adversaries -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, _, _ in cases.STRIDE_FIELDS])
def test_the_stride_gives_the_plain_records(built, name):
    """64^3, single-voxel obstacles at 0.2 %, 4096 random segments and 5120 aimed at an obstacle or past it by one voxel, each
    walked away from the obstacle and towards it, lo
    over squares and non-squares: the stride's records are the plain walk's and the model's, in both modes."""
    vol, to_empty, outside, D, segments = cases.stride_case(name)
    field, _ = euclidean(vol, to_empty, outside)
    d_segments, n = device_words(segments), len(segments)
    import torch
    from cpuvoxelraycaster_amd import capi
    for touch in (False, True):
        visited = cases.stride_visited(touch)
        for lo in cases.STRIDE_LOS:
            want = model.records(visited, D, lo, NONE)
            for plain in (False, True):
                d_out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
                field.sightDevice(n, d_segments.data_ptr(), d_out.data_ptr(), lo, NONE, touch, plain)
                got = d_out.cpu().numpy().view(capi.SIGHT_DTYPE)
                assert got.tobytes() == want.tobytes(), (name, lo, touch, plain, [(i, segments[i], got[i], want[i]) for i in np.flatnonzero(got != want)[:3]])
    # host memory once: the staged form of the same call
    assert field.sight(segments[:, :3], segments[:, 3:], 5, NONE, True).tobytes() == model.records(cases.stride_visited(True), D, 5, NONE).tobytes()
    field.close()


# ---- 4. no stride: a band with an upper end, travel fields ----------------------------------------------------------------

def test_a_band_and_travel_fields_take_the_plain_walk(built):
    S = 16
    vol = cases.random_solid(S, 0.03, 104)
    field, D = euclidean(vol)
    rng = np.random.default_rng(6)
    segments = rng.integers(0, S, (600, 6)).astype(np.int32)
    for touch in (False, True):
        want = model.sight(D, S, segments, 4, 100, touch)
        assert {int(s) for s in want["status"]} == {model.CLEAR, model.BLOCKED}
        every_way(field, segments, 4, 100, touch, want)
    field.close()
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[tuple(np.argwhere(vol == 0)[0])] = 1
    volume, seed_volume = volume_of(vol), volume_of(seeds)
    for connectivity in (6, 26):
        travel = volume.travelField(seed_volume, connectivity, through_empty=True)
        T = travel_model.field(vol, seeds, connectivity, True)
        assert np.array_equal(travel.download(), T) and travel.connectivity == connectivity
        for touch in (False, True):
            want = model.sight(T, S, segments, 0, NONE - 1, touch)
            assert {int(s) for s in want["status"]} == {model.CLEAR, model.BLOCKED}
            every_way(travel, segments, 0, NONE - 1, touch, want)
        travel.close()
    volume.close()
    seed_volume.close()


# ---- 5. an all-NONE field ---------------------------------------------------------------------------------------------

def test_an_all_none_field(built):
    S = 32
    field, D = euclidean(np.zeros((S, S, S), np.uint8))
    assert (D == NONE).all()
    segments = np.random.default_rng(7).integers(0, S, (300, 6)).astype(np.int32)
    for touch in (False, True):
        clear = model.sight(D, S, segments, 1, NONE, touch)
        assert (clear["status"] == model.CLEAR).all()
        every_way(field, segments, 1, NONE, touch, clear)
        blocked = model.sight(D, S, segments, 0, NONE - 1, touch)
        assert (blocked["status"] == model.BLOCKED).all() and np.array_equal(blocked["at"], segments[:, :3]) and np.array_equal(blocked["before"], segments[:, :3])
        every_way(field, segments, 0, NONE - 1, touch, blocked)
    field.close()


# ---- 6. edges ---------------------------------------------------------------------------------------------------------

def test_edges_and_refusals(built):
    from cpuvoxelraycaster_amd import capi
    S = 8
    vol = cases.random_solid(S, 0.1, 106)
    field, D = euclidean(vol)
    L = capi.load()
    # a == b, clear and blocked
    same = np.concatenate([np.argwhere(vol == 0)[:5], np.argwhere(vol)[:5]])
    segments = np.concatenate([same, same], 1).astype(np.int32)
    want = model.sight(D, S, segments, 1, NONE)
    assert np.array_equal(want["at"], same) and np.array_equal(want["before"], same) and list(want["status"]) == [model.CLEAR] * 5 + [model.BLOCKED] * 5
    every_way(field, segments, 1, NONE, True, want)
    # an endpoint outside on each side of each axis: OUTSIDE, every other byte 0
    outside = []
    for axis in range(3):
        for value in (-1, S, -2 ** 31, 2 ** 31 - 1):
            for end in (0, 3):
                seg = [1, 2, 3, 4, 5, 6]
                seg[end + axis] = value
                outside.append(seg)
    outside = np.array(outside, np.int32)
    want = model.sight(D, S, outside, 1, NONE)
    assert (want["status"] == model.OUTSIDE).all() and not want["at"].any() and not want["before"].any()
    every_way(field, outside, 1, NONE, False, want)
    # n = 1000: more than one workgroup and not a multiple of it, with guard records behind `out`
    many = np.random.default_rng(8).integers(-1, S + 1, (1000, 6)).astype(np.int32)
    want = model.sight(D, S, many, 1, NONE, True)
    assert {int(s) for s in want["status"]} == {model.CLEAR, model.BLOCKED, model.OUTSIDE}
    assert device_sight(field, many, 1, NONE, True, False, guard=24).tobytes() == want.tobytes()
    # n = 0: a no-op, NULL buffers allowed
    assert L.vrc_sight_segments(field._h, 0, None, 1, NONE, 0, None, capi.VRC_MEM_HOST, None) == 0
    assert len(field.sight(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    # refusals
    out, segs = np.zeros(1, capi.SIGHT_DTYPE), np.zeros((1, 6), np.int32)
    for args, text in (((1, None, 1, NONE, 0, capi.ptr(out), 0, None), b"null buffer"), ((1, capi.ptr(segs), 1, NONE, 0, None, 0, None), b"null buffer"),
                       ((1, capi.ptr(segs), 5, 4, 0, capi.ptr(out), 0, None), b"lo 5 above hi 4"), ((1, capi.ptr(segs), 1, NONE, 4, capi.ptr(out), 0, None), b"unknown flag bits"),
                       ((1, capi.ptr(segs), 1, NONE, 0, capi.ptr(out), 2, None), b"bad mem kind 2"),
                       ((0x7fffffff * 256 + 1, capi.ptr(segs), 1, NONE, 0, capi.ptr(out), 0, None), b"too many segments")):
        assert L.vrc_sight_segments(field._h, *args) == -1 and text in L.vrc_last_error(), text
    handle, eye, zero = C.c_void_p(), np.array([0, S, 0], np.uint32), np.zeros(3, np.uint32)
    for args, text in (((capi.ptr(eye), 0, 1, NONE, 0, C.byref(handle), None), b"outside the volume"), ((capi.ptr(zero), 0, 5, 4, 0, C.byref(handle), None), b"lo 5 above hi 4"),
                       ((capi.ptr(zero), 0, 1, NONE, 8, C.byref(handle), None), b"unknown flag bits"), ((capi.ptr(zero), 0, 1, NONE, 0, None, None), b"null argument")):
        assert L.vrc_sight_field(field._h, *args) == -1 and text in L.vrc_last_error() and not handle.value, text
    field.close()


# ---- 7. 512^3 -----------------------------------------------------------------------------------------------------------

def test_the_far_corner_at_512(built):
    """A few voxels set near the far corner of 512^3 and 64 segments there, where dense indices exceed 2^26 (the last is 2^27
    - 1); the model reads its values through vrc_distance_at, so no 512 MiB field comes to the host.  Depth 10, where the byte
    offset passes 2^32, is not run: the field alone is 4 GiB.  The index width is checked by reading: csrc/vrc_sight.hip
    forms ((x << depth | y) << depth | z) in size_t before it scales by 4."""
    import cpuvoxelraycaster_amd as vrc
    S = 512
    volume = vrc.VoxelVolume(9)
    solid = np.array([[500, 500, 500], [505, 498, 503], [490, 509, 507], [510, 510, 510]], np.uint32)
    volume.setVoxels(solid)
    field = volume.distanceField()
    volume.close()
    rng = np.random.default_rng(9)
    segments = np.concatenate([rng.integers(470, S, (60, 6)), [[470, 470, 470, 511, 511, 511], [511, 511, 511, 400, 440, 480], [500, 500, 490, 500, 500, 511],
                                                               [511, 0, 511, 511, 511, 511]]]).astype(np.int32)
    assert len(segments) == 64
    cache = {}

    def at(p):
        if p not in cache:
            cache[p] = int(field.at(np.array([p], np.uint32))[0])
        return cache[p]

    # every voxel any walk visits, read in one call
    voxels = sorted({p for s in segments for p in model.walk(s[:3], s[3:], True)})
    cache.update(zip(voxels, (int(v) for v in field.at(np.array(voxels, np.uint32)))))
    assert at((500, 500, 500)) == 0 and at((511, 511, 511)) == 3
    for lo in (1, 10):
        for touch in (False, True):
            want = model.sight(at, S, segments, lo, NONE, touch)
            every_way(field, segments, lo, NONE, touch, want)
        assert {int(s) for s in want["status"]} == {model.CLEAR, model.BLOCKED}
    field.close()


# ---- 8. the sight field ---------------------------------------------------------------------------------------------

def check_sight_field(field, D, vol, eye, radius, lo, touch):
    want = model.sight_field(D, eye, radius, lo, NONE, touch)
    seen = field.visibleFrom(eye, radius, lo, NONE, touch)
    got = seen.download()
    assert np.array_equal(got, want), (eye, radius, lo, touch, np.argwhere(got != want)[:3])
    visible, max_d2, argmax = model.field_stats(want)
    assert (seen.stats.visible, seen.stats.max_d2, tuple(seen.stats.argmax), seen.stats.reserved) == (visible, max_d2, argmax, 0)
    assert seen.connectivity == 0 and seen.depth == field.depth and seen.bytes() == field.bytes()
    plain = field.visibleFrom(eye, radius, lo, NONE, touch, plain=True)
    again = field.visibleFrom(eye, radius, lo, NONE, touch)
    assert plain.download().tobytes() == got.tobytes() == again.download().tobytes()           # two calls give identical bytes
    # select of the result, AND-ed with the solid: the visible blocks
    picked = seen.select(0, NONE - 1)
    assert np.array_equal(picked.download() & vol, ((want != NONE) & (vol != 0)).astype(np.uint8))
    for handle in (picked, plain, again, seen):
        handle.close()
    return want


def test_the_sight_field_whole_at_16(built):
    S = 16
    vol = cases.random_solid(S, 0.05, 108)
    vol[8, 8, 8] = 0
    field, D = euclidean(vol)
    for touch in (False, True):
        want = check_sight_field(field, D, vol, (8, 8, 8), 0, 1, touch)                         # the eye in the open
        assert 200 < (want != NONE).sum() < S ** 3 and (want[vol != 0] != NONE).any()
    check_sight_field(field, D, vol, (0, 15, 3), 0, 2, False)
    wall = tuple(int(v) for v in np.argwhere(vol)[3])                                          # the eye in a wall: only the eye is finite
    want = check_sight_field(field, D, vol, wall, 0, 1, True)
    assert (want != NONE).sum() == 1 and want[wall] == 0
    volume = volume_of(vol)
    seen = volume.visibleFrom((8, 8, 8))
    assert np.array_equal(seen.download(), (model.sight_field(D, (8, 8, 8), 0, 1, NONE) != NONE).astype(np.uint8))
    seen.close()
    volume.close()
    field.close()


def test_the_sight_field_within_a_radius_at_32(built):
    S = 32
    vol = cases.random_solid(S, 0.02, 109)
    vol[20, 12, 16] = 0
    field, D = euclidean(vol)
    want = check_sight_field(field, D, vol, (20, 12, 16), 10, 1, False)
    assert want.max() == NONE and want[want != NONE].max() <= 100 and 1000 < (want != NONE).sum()
    check_sight_field(field, D, vol, (20, 12, 16), 10, 1, True)
    field.close()


def test_a_sight_field_is_walked_plainly(built):
    """A sight field has connectivity 0 like a Euclidean field, but it is no distance to a set: NONE in every shadow, small
    values round the eye.  hi = NONE on it -- does this path stay out of what the guard sees within r -- must not stride:
    the records with and without VRC_SIGHT_PLAIN are the model's, and so is a sight field made from a sight field."""
    S = 16
    vol = cases.random_solid(S, 0.05, 110)
    vol[8, 8, 8] = 0
    field, D = euclidean(vol)
    seen = field.visibleFrom((8, 8, 8))
    V = model.sight_field(D, (8, 8, 8), 0, 1, NONE)
    assert np.array_equal(seen.download(), V) and seen.connectivity == 0 and (V == NONE).sum() > 100
    segments = np.random.default_rng(10).integers(0, S, (2000, 6)).astype(np.int32)
    for lo in (1, 5):
        for touch in (False, True):
            want = model.sight(V, S, segments, lo, NONE, touch)
            assert {int(s) for s in want["status"]} == {model.CLEAR, model.BLOCKED}
            every_way(seen, segments, lo, NONE, touch, want)
    for touch in (False, True):
        check_sight_field(seen, V, vol, (2, 3, 13), 0, 5, touch)
    seen.close()
    field.close()


# ---- 9. smoothPath ----------------------------------------------------------------------------------------------------

def test_smooth_path_round_a_wall(built):
    import cpuvoxelraycaster_amd as vrc
    solid, a, b = cases.wall_case(32)
    volume = volume_of(solid)
    route = volume.shortestPath(a, b, connectivity=6)
    field = volume.distanceField()
    assert route is not None and not volume.lineOfSight(a, b) and volume.lineOfSight(a, (a[0] + 5, a[1], a[2])) and not volume.lineOfSight(a, (32, 0, 0))
    D, rows = distance_model.field(solid), [tuple(p) for p in route]
    for radius in (0, 1):
        way = vrc.smoothPath(route, field, radius)
        assert tuple(way[0]) == a and tuple(way[-1]) == b and 2 < len(way) <= len(route)
        # a subsequence of the route
        at, index = 0, []
        for p in way:
            at = rows.index(tuple(p), at) + 1
            index.append(at - 1)
        lo = radius * radius + 1
        legs = field.sight(way[:-1], way[1:], lo, NONE, True)
        assert model.sight(D, 32, np.concatenate([way[:-1], way[1:]], 1), lo, NONE, True).tobytes() == legs.tobytes()
        # every leg is CLEAR, or it is one step of the route that is not clear itself: nothing to pull straight there
        single = np.diff(index) == 1
        assert ((legs["status"] == model.CLEAR) | single).all()
        if radius == 0:                                                    # a 6-step route through the air: every leg is CLEAR
            assert (legs["status"] == model.CLEAR).all() and len(way) < len(route) // 4
    field.close()
    volume.close()
