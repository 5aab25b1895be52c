"""vrc_morph_apply on the device (include/vrc.h) against the numpy model of morph_model.py, bit for bit after download().  The
sizes are the smallest at which each hazard of csrc/vrc_morph.hip first appears: 4^3 two brick rows in a word and every
element reaching outside, 8^3 one word per row, 16^3 the first z-neighbour words, 32^3 a reach of 16 that crosses two words
along z and eight brick rows, 64^3 words whose whole reach-16 neighbourhood lies inside, several tiles and workgroups."""

import numpy as np
import pytest

import morph_model as model
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu

SIZES = [4, 8, 16, 32, 64]
COMBOS = [(what, of, outside) for what in (model.DILATE, model.ERODE) for of in (model.SOLID, model.EMPTY) for outside in (0, 1)]


def depth_of(S):
    return S.bit_length() - 1


def differing(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:4].tolist()


def whole(S):
    return (0, 0, 0), (S, S, S), (0, 0, 0)


def garbage(S, which):
    """what a call finds in dst: nothing, everything, or a random set (the pattern of the cells test)"""
    if which == 0:
        return np.zeros((S, S, S), np.uint8)
    if which == 1:
        return np.ones((S, S, S), np.uint8)
    return (np.random.default_rng(S).random((S, S, S)) < 0.5).astype(np.uint8)


class Bench:
    """a source, a destination and the three patterns a destination starts from, all resident"""

    def __init__(self, vol):
        import cpuvoxelraycaster_amd as vrc
        self.S = vol.shape[0]
        self.vol, self.src, self.dst = vol, volume_of(vol, depth_of(self.S)), vrc.VoxelVolume(depth_of(self.S))
        self.before = [garbage(self.S, w) for w in range(3)]
        self.patterns = [volume_of(b, depth_of(self.S)) for b in self.before]
        self.calls = 0

    def check(self, e, what, of, outside, op=None, pattern=None, origin=None):
        """one host-memory call under `op` onto `pattern` (both cycle when not given) against the model"""
        op = self.calls % 3 if op is None else op
        pattern = (self.calls // 3) % 3 if pattern is None else pattern
        self.calls += 1
        self.dst.copyRegion(self.patterns[pattern], *whole(self.S))
        assert self.src.morph(what, e, self.dst, of == model.EMPTY, bool(outside), op, origin) is self.dst
        got, want = self.dst.download(), model.apply(self.before[pattern], self.vol, what, e, of, outside, op, origin)
        assert np.array_equal(got, want), (self.S, what, of, outside, op, pattern, np.asarray(e).reshape(-1, 3)[:6].tolist(), differing(got, want))

    def close(self):
        assert np.array_equal(self.src.download(), self.vol)         # the source is only read
        for v in [self.src, self.dst] + self.patterns:
            v.close()


# ---- 1. single offsets are translations ---------------------------------------------------------------------------------

def single_offsets():
    rng = np.random.default_rng(16)
    alone = [tuple(v if a == axis else 0 for a in range(3)) for axis in range(3) for v in range(-16, 17)]
    corners = [(x, y, z) for x in (-16, 15, 16) for y in (-15, 16, -16) for z in (16, -16, 15)]     # 27: signs and parities mixed
    return alone, corners, [tuple(t) for t in rng.integers(-16, 17, (200, 3)).tolist()]


@pytest.mark.parametrize("S", [32, 64])
def test_single_offsets_are_translations(built, S):
    alone, corners, random = single_offsets()
    assert len(alone) == 99 and len(corners) == 27 and len(set(corners)) == 27 and len(random) == 200
    vol = (np.random.default_rng(S).random((S, S, S)) < 0.3).astype(np.uint8)
    bench = Bench(vol)
    for outside in (0, 1):
        padded = np.pad(vol, 16, constant_values=outside)
        for e in alone + corners + random:
            bench.dst.copyRegion(bench.patterns[1], *whole(S))
            bench.src.morph(model.DILATE, [e], bench.dst, outside=bool(outside))
            got = bench.dst.download()
            want = padded[16 - e[0]:16 - e[0] + S, 16 - e[1]:16 - e[1] + S, 16 - e[2]:16 - e[2] + S]         # K(p) = A(p - e)
            assert np.array_equal(got, want), (S, outside, e, differing(got, want))
    bench.close()


@pytest.mark.parametrize("S,plane", [(4, None)] + [(8, x) for x in range(8)])
def test_one_voxel_by_every_small_offset(built, S, plane):
    """every offset in [-3, 3]^3 from a single solid voxel at every position (at 8^3 one x plane of positions per case): the
    result is the one voxel p + e, or nothing when that lies outside.  Device lists and the result read as a voxel list, so
    that nothing waits between the calls; every pair is still held to its own result."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    offsets = np.array([e for e in np.ndindex(7, 7, 7)], np.int32) - 3
    positions = [p for p in np.ndindex(S, S, S) if plane is None or p[0] == plane]
    t_offsets = torch.from_numpy(offsets).cuda()
    found = torch.full((len(positions), len(offsets), 2, 3), 0x7B7B7B7B, dtype=torch.int32).cuda()
    totals = torch.full((len(positions), len(offsets)), -1, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    src, dst = vrc.VoxelVolume(depth_of(S)), vrc.VoxelVolume(depth_of(S))
    with Stream() as stream:
        for i, p in enumerate(positions):
            src.setVoxels([p])
            for j in range(len(offsets)):
                src.morphDevice(dst, model.DILATE, 1, t_offsets.data_ptr() + 12 * j, stream=stream)
                dst.extractVoxelsDevice(capi.VRC_VOXELS_ALL, capi.VRC_VOXELS_XYZ, 0, 2, found.data_ptr() + 24 * (i * len(offsets) + j),
                                        totals.data_ptr() + 8 * (i * len(offsets) + j), stream=stream)
            capi.check(capi.load().vrc_stream_synchronize(0, stream))      # the calls only read src: nothing else orders the next edit behind them
            src.setVoxels([p], False)
    q = np.array(positions, np.int64)[:, None, :] + offsets.astype(np.int64)[None, :, :]
    inside = ((q >= 0) & (q < S)).all(axis=2)
    assert np.array_equal(totals.cpu().numpy(), inside.astype(np.int64))
    got = found.cpu().numpy()
    assert np.array_equal(got[:, :, 0, :][inside], q[inside]) and (got[:, :, 0, :][~inside] == 0x7B7B7B7B).all() and (got[:, :, 1, :] == 0x7B7B7B7B).all()
    src.close()
    dst.close()


# ---- 2. elements --------------------------------------------------------------------------------------------------------

def named_elements():
    out = [model.ball(r) for r in range(6)]
    out += [model.box(3, 3, 3), model.box(2, 2, 2), model.box(3, 5, 3, (0, 4, 1)), model.box(4, 1, 2, (3, 0, 0)), model.box(1, 2, 7, (0, 1, 6)), model.cross()]
    for axis in range(3):
        out += [model.line(axis, 0, 0), model.line(axis, -3, 4), model.line(axis, -4, 4), model.line(axis, -16, 16)]
    return out


@pytest.mark.parametrize("S", SIZES)
def test_elements(built, S):
    rng = np.random.default_rng(100 + S)
    bench = Bench(model.source(S))
    for e in named_elements():
        for what, of, outside in COMBOS:
            bench.check(e, what, of, outside)
    for i in range(40):                                            # sparse: 1 to 200 offsets over the whole reach, two forms each
        e = model.random_element(rng, int(rng.integers(1, 201)))
        for what, of, outside in (COMBOS[i % 8], COMBOS[(i + 3) % 8]):
            bench.check(e, what, of, outside)
    assert bench.calls == 8 * 24 + 80
    bench.close()


@pytest.mark.parametrize("S", SIZES)
def test_degenerate_elements_and_every_op(built, S):
    rng = np.random.default_rng(S)
    bench = Bench(model.source(S))
    zero = np.zeros((1, 3), np.int32)
    tripled = np.repeat(model.random_element(rng, 30, 6), 3, axis=0)
    rng.shuffle(tripled)
    for e in (np.zeros((0, 3), np.int32), zero, tripled):
        for what, of, outside in COMBOS:
            for op in (model.REPLACE, model.OR, model.ANDNOT):
                for pattern in range(3):
                    bench.check(e, what, of, outside, op, pattern)
    # the zero offset alone is a copy, and of the empty set the complement; n == 0 is nothing, or everything
    assert np.array_equal(model.morph(bench.vol, model.ERODE, zero), bench.vol) and np.array_equal(model.morph(bench.vol, model.DILATE, zero, model.EMPTY), 1 - bench.vol)
    assert model.morph(bench.vol, model.DILATE, [], outside=1).sum() == 0 and model.morph(bench.vol, model.ERODE, [], model.EMPTY).sum() == S ** 3
    # an origin: a list of voxel coordinates about a pivot
    e = model.box(2, 3, 2) + np.array([9, 1, 30], np.int32)
    bench.check(e.astype(np.uint32).view(np.int32), model.DILATE, model.SOLID, 0, origin=(9, 1, 30))
    bench.check(e, model.ERODE, model.EMPTY, 1, origin=(8, 2, 29))
    bench.close()


def test_the_whole_cube(built):
    """all 33^3 offsets: every column of the table, every bit of every mask"""
    S = 16
    cube = model.box(33, 33, 33)
    assert len(cube) == 35937 and cube.min() == -16 and cube.max() == 16
    vol = np.zeros((S, S, S), np.uint8)
    vol[5, 9, 2] = 1
    bench = Bench(vol)
    bench.check(cube, model.DILATE, model.SOLID, 0, model.REPLACE, 2)            # one voxel reaches everywhere
    bench.check(cube, model.ERODE, model.EMPTY, 1, model.REPLACE, 2)             # and one solid voxel spoils every pivot
    bench.check(cube, model.ERODE, model.SOLID, 1, model.OR, 0)
    bench.check(cube, model.DILATE, model.EMPTY, 0, model.ANDNOT, 1)
    bench.close()


# ---- 3. against code that exists ---------------------------------------------------------------------------------------

def same_on_device(a, b):
    delta = a.diff(b)
    words = int(delta.stats.words)
    delta.close()
    return words == 0


def test_ball_is_the_distance_field(built):
    import cpuvoxelraycaster_amd as vrc
    S = 32
    world = volume_of(model.source(S), 5)
    for r in range(1, 6):
        grown, by_ball = world.clone().dilate(r), world.morph(model.DILATE, vrc.element_ball(r))
        assert same_on_device(grown, by_ball), r
        assert same_on_device(world.clone().dilateBy(vrc.element_ball(r)), grown)
        for open_border in (False, True):
            shrunk, by_ball = world.clone().erode(r, open_border), world.morph(model.ERODE, vrc.element_ball(r), outside=not open_border)
            assert same_on_device(shrunk, by_ball), (r, open_border)
            assert same_on_device(world.clone().erodeBy(vrc.element_ball(r), open_border), shrunk)
    assert same_on_device(world.clone().openShape(2), world.clone().openBy(vrc.element_ball(2)))
    assert same_on_device(world.clone().closeShape(2), world.clone().closeBy(vrc.element_ball(2)))
    assert not same_on_device(world.clone().dilate(2), world)
    world.close()


@pytest.mark.parametrize("S", SIZES)
def test_cube_and_cross_are_the_automaton(built, S):
    import cpuvoxelraycaster_amd as vrc
    world = volume_of(model.source(S), depth_of(S))
    for outside in (False, True):
        assert same_on_device(world.morph(model.DILATE, vrc.element_box(3, 3, 3), outside=outside), world.cellStep(range(1, 27), range(0, 27), 26, outside))
        assert same_on_device(world.morph(model.DILATE, vrc.element_cross(), outside=outside), world.cellStep(range(1, 7), range(0, 7), 6, outside))
        # the erosion: a voxel stays when all 26 (6) neighbours are solid
        assert same_on_device(world.morph(model.ERODE, vrc.element_box(3, 3, 3), outside=outside), world.cellStep(0, 1 << 26, 26, outside))
        assert same_on_device(world.morph(model.ERODE, vrc.element_cross(), outside=outside), world.cellStep(0, 1 << 6, 6, outside))
    world.close()


@pytest.mark.parametrize("S", SIZES)
def test_duality_on_the_device(built, S):
    import cpuvoxelraycaster_amd as vrc
    rng = np.random.default_rng(S)
    world = volume_of(model.source(S), depth_of(S))
    for e in (model.box(3, 2, 4, (2, 0, 1)), model.random_element(rng, 60), model.line(2, 3, 16)):
        for of_empty in (False, True):
            for outside in (False, True):
                eroded = world.morph(model.ERODE, e, of_empty=of_empty, outside=outside)
                dual = world.morph(model.DILATE, vrc.reflect(e), of_empty=not of_empty, outside=not outside)
                complement = dual.morph(model.DILATE, [(0, 0, 0)], of_empty=True)
                assert same_on_device(eroded, complement), (S, of_empty, outside)
                assert np.array_equal(eroded.download(), 1 - dual.download())
    world.close()


# ---- 4. the list in device memory ---------------------------------------------------------------------------------------

def test_a_piece_becomes_an_element_on_the_device(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    S = 32
    shape = np.zeros((16, 16, 16), np.uint8)
    shape[3:8, 4, 2:11] = shape[5, 4:9, 6] = shape[7, 7, 7] = shape[1, 1, 15] = 1
    pivot = (5, 4, 6)
    n = int(shape.sum())
    piece, world, dst = volume_of(shape, 4), volume_of(model.source(S), 5), vrc.VoxelVolume(5)
    for what, of_empty, outside in [(model.DILATE, False, False), (model.ERODE, True, False), (model.ERODE, False, True)]:
        buffer = torch.full((n + 2, 3), 0x7B7B7B7B, dtype=torch.int32).cuda()         # a canary row on either side of the list
        total = torch.zeros(1, dtype=torch.int64).cuda()
        torch.cuda.synchronize()
        with Stream() as stream:
            piece.extractVoxelsDevice(capi.VRC_VOXELS_ALL, capi.VRC_VOXELS_XYZ, 0, n, buffer.data_ptr() + 12, total.data_ptr(), stream=stream)
            assert world.morphDevice(dst, what, n, buffer.data_ptr() + 12, pivot, of_empty, outside, stream=stream) is dst
            got = dst.download()
        listed = buffer.cpu().numpy()
        assert total.item() == n and (listed[0] == 0x7B7B7B7B).all() and (listed[-1] == 0x7B7B7B7B).all()
        assert sorted(listed[1:-1].tolist()) == np.argwhere(shape).tolist()
        by_host = world.morph(what, vrc.element_of(shape, pivot), of_empty=of_empty, outside=outside)
        assert np.array_equal(got, by_host.download())
        assert np.array_equal(got, model.morph(model.source(S), what, np.argwhere(shape), model.EMPTY if of_empty else model.SOLID, int(outside), pivot))
        by_host.close()
    for v in (piece, world, dst):
        v.close()


def test_a_device_list_drops_what_is_out_of_reach(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 32
    lo, hi = -(1 << 31), (1 << 31) - 1
    good = model.random_element(np.random.default_rng(5), 40)
    bad = np.array([(17, 0, 0), (0, -17, 0), (0, 0, 17), (-17, 16, 16), (lo, 0, 0), (0, hi, 0), (1, 2, lo), (hi, hi, hi), (lo, lo, lo), (16, 16, -17)], np.int32)
    mixed = np.concatenate([good[:13], bad[:4], good[13:30], bad[4:], good[30:]])
    world, dst = volume_of(model.source(S), 5), vrc.VoxelVolume(5)
    scratch = (world.editScratchBytes(), dst.editScratchBytes())
    for origin in (None, (0, 0, 0), (3, -2, 1)):
        shift = np.zeros(3, np.int32) if origin is None else np.array(origin, np.int32)
        rows = np.full((len(mixed) + 2, 3), 0x7B7B7B7B, np.int32)
        rows[1:-1] = mixed
        near = (np.abs(mixed.astype(np.int64)) <= 17).all(axis=1)  # these move with the origin; INT32_MIN and INT32_MAX stay out of reach in 64 bits
        rows[1:-1][near] += shift
        assert sorted(model.in_reach(rows[1:-1].astype(np.int64) - shift).tolist()) == sorted(good.tolist()) and near.sum() == len(good) + 5
        t = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        for what, of, outside in COMBOS:
            with Stream() as stream:
                world.morphDevice(dst, what, len(mixed), t.data_ptr() + 12, origin, of == model.EMPTY, bool(outside), stream=stream)
                got = dst.download()
            want = model.morph(model.source(S), what, good, of, outside)
            assert np.array_equal(got, want), (origin, what, of, outside, differing(got, want))
        assert np.array_equal(t.cpu().numpy(), rows)               # the list and the canaries around it are only read
    assert (world.editScratchBytes(), dst.editScratchBytes()) == scratch
    world.close()
    dst.close()


# ---- 5. fitsAt, match, and the path of a shaped agent ---------------------------------------------------------------------

def test_fits_at_a_carved_room(built):
    import cpuvoxelraycaster_amd as vrc
    S = 32
    vol = np.ones((S, S, S), np.uint8)
    vol[10:13, 3:8, 20:23] = 0                                     # exactly 3 x 5 x 3
    vol[20:24, 11:17, 5:8] = 0                                     # 4 x 6 x 3: two by two pivots
    vol[0:3, 27:32, 29:32] = 0                                     # 3 x 5 x 3 in a corner of the volume
    vol[27:32, 0:3, 0:3] = 0                                       # 5 x 3 x 3: the shape does not turn
    world = volume_of(vol, 5)
    fits = world.fitsAt(vrc.element_box(3, 5, 3))
    want = [[1, 29, 30], [11, 5, 21], [21, 13, 6], [21, 14, 6], [22, 13, 6], [22, 14, 6]]
    assert np.argwhere(fits.download()).tolist() == want
    assert np.array_equal(fits.download(), model.fits_at(vol, model.box(3, 5, 3)))
    fits.close()
    world.close()


def test_match_finds_the_planted_staircases(built):
    import cpuvoxelraycaster_amd as vrc
    S = 32
    steps = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0)]
    air = [(0, 1, 0), (0, 2, 0), (1, 2, 0), (3, 2, 0), (-1, 0, 0)]
    vol = np.zeros((S, S, S), np.uint8)
    planted = [(0, 0, 0), (8, 20, 5), (20, 9, 31), (28, 29, 16), (14, 14, 14)]
    for p in planted:
        for s in steps:
            vol[p[0] + s[0], p[1] + s[1], p[2] + s[2]] = 1
    for p, missing in [((3, 12, 25), 2), ((22, 22, 3), 4)]:        # a staircase with a step missing
        for i, s in enumerate(steps):
            vol[p[0] + s[0], p[1] + s[1], p[2] + s[2]] = i != missing
    vol[9, 27, 9:12] = 1
    for s in steps:                                                # a staircase with a voxel where air has to be
        vol[25 + s[0], 2 + s[1], 20 + s[2]] = 1
    vol[25, 4, 20] = 1
    world = volume_of(vol, 5)
    found = world.match(steps, air)
    assert np.argwhere(found.download()).tolist() == sorted(list(p) for p in planted)
    assert np.array_equal(found.download(), model.match(vol, steps, air))
    walled = world.match(steps, air, outside=True)                 # beyond the faces solid: the one at x = 0 has no air at x = -1
    assert np.argwhere(walled.download()).tolist() == sorted(list(p) for p in planted[1:])
    for v in (found, walled, world):
        v.close()


def test_a_shaped_agent_passes_a_door_as_wide_as_itself(built):
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    S = 32
    agent = vrc.element_box(3, 3, 3)
    start, goal = (6, 6, 4), (20, 6, 4)
    for width, arrives in [(3, True), (2, False)]:
        vol = np.ones((S, S, S), np.uint8)
        vol[2:12, 2:12, 2:12] = 0                                  # two chambers
        vol[14:26, 2:12, 2:12] = 0
        vol[12:14, 5:5 + width, 3:6] = 0                           # and a door through the wall between them, 3 high
        world = volume_of(vol, 5)
        free = world.fitsAt(agent)
        assert free.download()[start] == 1 and free.download()[goal] == 1
        seeds = vrc.VoxelVolume(5)
        seeds.setVoxels([start])
        field = free.travelField(seeds, 6)                         # through the pivots at which the agent stands free
        steps = int(field.at([goal])[0])
        assert (steps != capi.VRC_DISTANCE_NONE) == arrives, (width, steps)
        if arrives:
            assert steps == goal[0] - start[0]                     # straight through the middle of the door
        one_voxel = world.travelField(seeds, 6, through_empty=True)          # an agent of one voxel passes either door
        assert int(one_voxel.at([goal])[0]) != capi.VRC_DISTANCE_NONE
        for thing in (field, one_voxel, seeds, free, world):
            thing.close()


# ---- 6. ordering --------------------------------------------------------------------------------------------------------

def test_morph_sees_an_edit_in_flight(built):
    """a device-memory setVoxels on a stream, then the call on the same stream and on another one: both run behind it"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 64
    rng = np.random.default_rng(64)
    base = (rng.random((S, S, S)) < 0.05).astype(np.uint8)
    extra = rng.integers(0, S, (200000, 3)).astype(np.uint32)
    edited = base.copy()
    edited[tuple(extra.T.astype(np.int64))] = 1
    e = model.box(2, 1, 3, (0, 0, 2))
    want = model.morph(edited, model.ERODE, e)
    assert not np.array_equal(want, model.morph(base, model.ERODE, e))
    t_extra, t_e = torch.from_numpy(extra.view(np.int32)).cuda(), torch.from_numpy(e).cuda()
    torch.cuda.synchronize()
    for other_stream in (False, True):
        src, dst = volume_of(base, 6), vrc.VoxelVolume(6)
        with Stream() as stream, Stream() as second:
            src.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
            dst.fillBoxes([[0, 0, 0, S, S, S]])
            src.morphDevice(dst, model.ERODE, len(e), t_e.data_ptr(), stream=second if other_stream else stream)
            got = dst.download()                                   # behind dst's last edit, the call
        assert np.array_equal(got, want), other_stream
        src.close()
        dst.close()


# ---- 7. scratch and refusals ----------------------------------------------------------------------------------------------

def test_scratch_is_unchanged_by_every_form(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 16
    world, dst = volume_of(model.source(S), 4), vrc.VoxelVolume(4)
    scratch = (world.editScratchBytes(), dst.editScratchBytes())
    ball = vrc.element_ball(2)
    t = torch.from_numpy(ball).cuda()
    world.morph(model.DILATE, ball, dst)
    world.morph(model.ERODE, [], dst, of_empty=True, outside=True, op=model.OR)
    world.morphDevice(dst, model.DILATE, len(ball), t.data_ptr())
    world.morphDevice(dst, model.ERODE, 0, None)
    dst.dilateBy(ball).erodeBy(ball, True).openBy(ball).closeBy(ball)
    for made in (world.fitsAt(ball), world.match(ball[:3], ball[3:5])):
        assert made.editScratchBytes() == scratch[1]
        made.close()
    assert (world.editScratchBytes(), dst.editScratchBytes()) == scratch
    assert np.array_equal(world.download(), model.source(S))
    world.close()
    dst.close()


def test_refusals_leave_dst_alone(built):
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    S = 8
    held = garbage(S, 2)
    src, dst, deeper = volume_of(model.source(S), 3), volume_of(held, 3), vrc.VoxelVolume(4)
    good = np.array([(1, 2, 3), (16, -16, 0)], np.int32)
    far = np.array([(1, 2, 3), (0, 0, 0), (0, -17, 4), (40, 0, 0)], np.int32)
    origin = np.array([0, 0, 1], np.int32)

    def call(d=dst, s=src, what=0, of=1, n=2, offsets=good, origin=None, outside=0, op=0, mem=0):
        return L.vrc_morph_apply(None if d is None else d._h, None if s is None else s._h, what, of, n, capi.ptr(offsets), capi.ptr(origin), outside, op, mem, None)

    refusals = [
        (dict(d=None), "null argument"),
        (dict(s=None), "null argument"),
        (dict(s=dst), "source and destination are the same volume"),
        (dict(s=deeper), "volumes of depths 3 and 4"),
        (dict(d=deeper), "volumes of depths 4 and 3"),
        (dict(what=2), "bad what 2"),
        (dict(of=3), "bad of 3"),
        (dict(of=0), "bad of 0"),
        (dict(outside=2), "outside 2 is neither 0 nor 1"),
        (dict(op=3), "bad op 3"),
        (dict(mem=2), "bad mem kind 2"),
        (dict(n=(1 << 20) + 1), "1048577 offsets, more than 1048576"),
        (dict(n=(1 << 20) + 1, mem=1), "1048577 offsets, more than 1048576"),
        (dict(offsets=None), "null offsets"),
        (dict(n=4, offsets=far), "offset 2 is (0, -17, 4) after the origin, beyond +-16"),
        (dict(n=4, offsets=far, origin=origin), "offset 2 is (0, -17, 3) after the origin, beyond +-16"),
        (dict(n=2, offsets=good, origin=origin * 2 - 1), "offset 1 is (17, -15, -1) after the origin, beyond +-16"),
    ]
    for kwargs, text in refusals:
        assert call(**kwargs) == -1                                # VRC_ERR_INVALID
        assert L.vrc_last_error() == ("vrc_morph_apply: " + text).encode(), kwargs
        assert np.array_equal(dst.download(), held) and deeper.solidCount() == 0
    assert call() == 0 and np.array_equal(dst.download(), model.morph(model.source(S), model.DILATE, good))       # the same call, legal
    with pytest.raises(vrc.VrcError, match="bad what 7"):
        src.morph(7, good)
    for v in (src, dst, deeper):
        v.close()
