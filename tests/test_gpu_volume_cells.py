"""The cell calls on the device (include/vrc.h: vrc_cells_step, vrc_cells_fill_random) against the numpy model of
cells_model.py, bit for bit after download().  The sizes are the smallest at which each hazard of csrc/vrc_cells.hip first
appears: 4^3 two brick rows in a word, 8^3 one word per row and no z-neighbour word, 16^3 the first z-neighbour words,
32^3 interior words with all 26 neighbour words present.  The step's launch takes a lane per word and the fill's a lane per
box word, neither is capped, so no size makes a lane take a second item; 128^3 is the many-workgroup case."""
import numpy as np
import pytest

import cells_model as model
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu

SIZES = [4, 8, 16, 32]


def depth_of(S):
    return S.bit_length() - 1


def differing(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:4].tolist()


def garbage(volume, S, which):
    """something for the step to overwrite: nothing, everything, or a random set"""
    volume.fillBoxes([[0, 0, 0, S, S, S]], which == 1)
    if which == 2:
        volume.setVoxels(np.argwhere(np.random.default_rng(S).random((S, S, S)) < 0.5))


# ---- 1. single counts: every plane of the adders and every leaf of the select trees ------------------------------------

@pytest.mark.parametrize("S", SIZES)
def test_single_counts(built, S):
    import cpuvoxelraycaster_amd as vrc
    vol = model.three_band(S)
    solid = vol != 0
    src, dst = volume_of(vol, depth_of(S)), vrc.VoxelVolume(depth_of(S))
    launches = 0
    for neighbours in (6, 26):
        for outside in (0, 1):
            c = model.counts(vol, neighbours, outside)
            for k in range(neighbours + 1):
                at_k = c == k
                for birth, survive, want in [(1 << k, 1 << k, at_k), (1 << k, 0, at_k & ~solid), (0, 1 << k, at_k & solid)]:
                    garbage(dst, S, launches % 3)
                    assert src.cellStep(birth, survive, neighbours, bool(outside), dst) is dst
                    got = dst.download()
                    assert np.array_equal(got, want), (S, neighbours, outside, k, birth, survive, differing(got, want))
                    launches += 1
    assert launches == 2 * 3 * (7 + 27)
    assert np.array_equal(src.download(), vol)                 # the source is only read
    src.close()
    dst.close()


def test_random_rules(built):
    """whole masks at once, and the model's count of changed voxels"""
    import cpuvoxelraycaster_amd as vrc
    rng = np.random.default_rng(26)
    for S in SIZES:
        vol = model.three_band(S)
        src, dst = volume_of(vol, depth_of(S)), vrc.VoxelVolume(depth_of(S))
        for neighbours in (6, 26):
            for outside in (0, 1):
                for _ in range(4):
                    legal = (2 << neighbours) - 1
                    birth, survive = int(rng.integers(0, 1 << 32)) & legal, int(rng.integers(0, 1 << 32)) & legal
                    want, changed = model.step(vol, birth, survive, neighbours, outside)
                    _, got_changed = src.cellStep(birth, survive, neighbours, bool(outside), dst, count_changed=True)
                    got = dst.download()
                    assert np.array_equal(got, want) and got_changed == changed, (S, neighbours, outside, hex(birth), hex(survive), got_changed, changed)
        src.close()
        dst.close()


# ---- 2. every shift at every bit: one solid voxel, birth at count 1 -------------------------------------------------------

def single_voxel_cases(S):
    if S <= 8:
        return [tuple(p) for p in np.indices((S, S, S)).reshape(3, -1).T.tolist()]
    e = S - 1
    rng = np.random.default_rng(S)
    corners = [(x, y, z) for x in (0, e) for y in (0, e) for z in (0, e)]
    seam = [(int(x), int(y), z) for z in (7, 8) for x, y in rng.integers(0, S, (6, 2))] + [(0, 0, 7), (e, e, 8), (1, 0, 8), (e - 1, e, 7)]
    return corners + seam + [tuple(p) for p in rng.integers(0, S, (200, 3)).tolist()]


@pytest.mark.parametrize("S", SIZES)
def test_one_voxel_at_every_position(built, S):
    import cpuvoxelraycaster_amd as vrc
    src, dst = vrc.VoxelVolume(depth_of(S)), vrc.VoxelVolume(depth_of(S))
    grid = np.indices((S, S, S))
    for p in single_voxel_cases(S):
        src.setVoxels([p])
        d = np.abs(grid - np.array(p).reshape(3, 1, 1, 1))
        for neighbours in (26, 6):
            # exactly the clipped neighbourhood: the voxels one step away, the centre not (it has no solid neighbour)
            want = ((d.max(axis=0) == 1) if neighbours == 26 else (d.sum(axis=0) == 1)).astype(np.uint8)
            _, changed = src.cellStep(1 << 1, 0, neighbours, False, dst, count_changed=True)
            got = dst.download()
            assert np.array_equal(got, want), (S, p, neighbours, differing(got, want))
            assert changed == int(want.sum()) + 1
        src.setVoxels([p], False)
    assert src.solidCount() == 0
    src.close()
    dst.close()


# ---- 3. borders -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", SIZES)
def test_full_volume_and_its_faces(built, S):
    import cpuvoxelraycaster_amd as vrc
    src, dst = vrc.VoxelVolume(depth_of(S)), vrc.VoxelVolume(depth_of(S))
    src.fillBoxes([[0, 0, 0, S, S, S]])
    interior = np.zeros((S, S, S), np.uint8)
    interior[1:S - 1, 1:S - 1, 1:S - 1] = 1
    for neighbours in (26, 6):
        _, changed = src.cellStep(0, 1 << neighbours, neighbours, True, dst, count_changed=True)
        assert dst.solidCount() == S ** 3 and changed == 0                      # beyond the faces solid: full stays full
        _, changed = src.cellStep(0, 1 << neighbours, neighbours, False, dst, count_changed=True)
        assert np.array_equal(dst.download(), interior) and changed == S ** 3 - (S - 2) ** 3
    # an empty volume with solid surroundings: birth at count 9 (a face of 26) / 1 (a face of 6) gives the face layer without its edges
    src.fillBoxes([[0, 0, 0, S, S, S]], False)
    c26, c6 = model.counts(np.zeros((S, S, S), np.uint8), 26, 1), model.counts(np.zeros((S, S, S), np.uint8), 6, 1)
    src.cellStep(1 << 9, 0, 26, True, dst)
    assert np.array_equal(dst.download(), c26 == 9)
    src.cellStep(1 << 1, 0, 6, True, dst)
    assert np.array_equal(dst.download(), c6 == 1)
    src.close()
    dst.close()


# ---- 4. changed -------------------------------------------------------------------------------------------------------

def test_changed_in_host_and_device_memory(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    for S in SIZES:
        vol = model.three_band(S)
        src, dst = volume_of(vol, depth_of(S)), vrc.VoxelVolume(depth_of(S))
        everything = (2 << 26) - 1
        rules = [(0x1E0, 0x7FF0, 26, 1), (1 << 3, 0x7C, 6, 0),
                 (everything, 0, 26, 0),                         # inverts every voxel
                 (0, everything, 26, 0), (0, 0x7F, 6, 1)]        # changes nothing
        for birth, survive, neighbours, outside in rules:
            want, changed = model.step(vol, birth, survive, neighbours, outside)
            scratch = (src.editScratchBytes(), dst.editScratchBytes())
            _, got = src.cellStep(birth, survive, neighbours, bool(outside), dst, count_changed=True)
            assert got == changed, (S, hex(birth), hex(survive), got, changed)
            assert (src.editScratchBytes(), dst.editScratchBytes()) == scratch          # the host-memory counter is staged in a block of the call's own
            counter = torch.full((3,), 0x7B7B7B7B7B7B7B7B, dtype=torch.int64).cuda()      # stale content and two canaries
            torch.cuda.synchronize()
            with Stream() as stream:
                src.cellStepDevice(dst, birth, survive, counter.data_ptr() + 8, neighbours, bool(outside), stream)
            assert counter.cpu().tolist() == [0x7B7B7B7B7B7B7B7B, changed, 0x7B7B7B7B7B7B7B7B]
            assert np.array_equal(dst.download(), want)
            # no counter: the asynchronous form, whatever `mem` says
            garbage(dst, S, 1)
            capi.check(capi.load().vrc_cells_step(dst._h, src._h, neighbours, birth, survive, outside, None, 77, None))
            assert np.array_equal(dst.download(), want)
        assert [r for r in rules if model.step(vol, *r)[1] == S ** 3] == [rules[2]] and model.step(vol, *rules[3])[1] == 0
        src.close()
        dst.close()


# ---- 5. iteration -----------------------------------------------------------------------------------------------------

def test_five_steps_ping_pong(built):
    import cpuvoxelraycaster_amd as vrc
    for S, (birth, survive, neighbours, outside) in [(16, (1 << 5, 0x30, 26, 0)), (32, (0x1E0, 0x7FF0, 26, 1)), (4, (1 << 2, 0x1C, 6, 0))]:
        state = model.three_band(S)
        a, b = volume_of(state, depth_of(S)), vrc.VoxelVolume(depth_of(S))
        for _ in range(5):
            state, _ = model.step(state, birth, survive, neighbours, outside)
            a.cellStep(birth, survive, neighbours, bool(outside), b)            # asynchronous: ordered by the volumes' last edits
            a, b = b, a
        assert np.array_equal(a.download(), state), S
        a.close()
        b.close()


def test_automaton_stops_at_the_fixed_point(built):
    S = 32
    vol = model.three_band(S)
    want, taken = model.automaton(vol, 100, model.SMOOTH_BIRTH, model.SMOOTH_SURVIVE, 26, 0)
    assert 5 < taken < 100 and 0 < want.sum()
    volume = volume_of(vol, 5)
    before = volume.editScratchBytes()
    assert volume.automaton(100, range(14, 27), range(13, 27)) == taken
    assert np.array_equal(volume.download(), want)
    assert volume.automaton(100, range(14, 27), range(13, 27)) == 0 and np.array_equal(volume.download(), want)
    assert volume.editScratchBytes() == before
    # an odd and an even number of steps short of it: the result lands in the volume either way
    for steps in (1, 2, 3):
        volume.close()
        volume = volume_of(vol, 5)
        assert volume.automaton(steps, model.SMOOTH_BIRTH, model.SMOOTH_SURVIVE) == steps
        assert np.array_equal(volume.download(), model.automaton(vol, steps, model.SMOOTH_BIRTH, model.SMOOTH_SURVIVE)[0]), steps
    assert volume.automaton(0, 1, 1) == 0
    volume.close()


# ---- 6. ordering ------------------------------------------------------------------------------------------------------

def test_step_sees_an_edit_in_flight(built):
    """a device-memory setVoxels on a stream, then the step on the same stream and on another one: both run behind it"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 64
    rng = np.random.default_rng(64)
    base = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
    extra = rng.integers(0, S, (200000, 3)).astype(np.uint32)
    edited = base.copy()
    edited[tuple(extra.T.astype(np.int64))] = 1
    want, changed = model.step(edited, 0x1E0, 0x7FF0, 26, 0)
    assert not np.array_equal(want, model.step(base, 0x1E0, 0x7FF0, 26, 0)[0])
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    counter = torch.zeros(1, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    for other_stream in (False, True):
        src, dst = volume_of(base, 6), vrc.VoxelVolume(6)
        with Stream() as stream, Stream() as second:
            src.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
            src.cellStepDevice(dst, 0x1E0, 0x7FF0, counter.data_ptr(), 26, False, second if other_stream else stream)
            got = dst.download()                                   # behind dst's last edit, the step
        assert np.array_equal(got, want), other_stream
        assert counter.cpu().tolist() == [changed]
        src.close()
        dst.close()


# ---- 7. a larger volume: many workgroups, rows of 16 words ---------------------------------------------------------------

def test_128_cubed(built):
    import cpuvoxelraycaster_amd as vrc
    S = 128
    src, dst = vrc.VoxelVolume(7), vrc.VoxelVolume(7)
    src.fillRandom(19, 0.4)
    vol = model.random_set(19, model.threshold_of(0.4), S)
    got = src.download()
    assert np.array_equal(got, vol), differing(got, vol)
    for birth, survive, neighbours, outside in [(0x3E00, 0x7FFF800, 26, 1), (0x18, 0x7C, 6, 0)]:
        want, changed = model.step(vol, birth, survive, neighbours, outside)
        _, got_changed = src.cellStep(birth, survive, neighbours, bool(outside), dst, count_changed=True)
        got = dst.download()
        assert np.array_equal(got, want) and got_changed == changed, (neighbours, differing(got, want), got_changed, changed)
    src.close()
    dst.close()


# ---- 8. the seeded fill -----------------------------------------------------------------------------------------------

BOXES = {4: [(1, 0, 1, 4, 3, 2), (0, 1, 3, 1, 2, 4), (3, 3, 0, 9, 9, 9)],
         8: [(1, 1, 1, 7, 6, 5), (2, 4, 3, 3, 5, 4)],
         16: [(1, 3, 5, 14, 9, 12), (2, 2, 9, 4, 4, 14), (5, 7, 8, 6, 8, 9)],                    # odd bounds; inside one word; one voxel
         32: [(3, 5, 7, 30, 21, 18), (6, 8, 17, 8, 10, 23), (31, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 1), (0, 0, 0, 32, 32, 32)]}


@pytest.mark.parametrize("S", SIZES)
def test_fill_random(built, S):
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    depth = depth_of(S)
    base = model.three_band(S)                                # a non-empty volume for the three ops to meet
    for density in (0.0, 0.12, 0.5, 1.0):
        volume = vrc.VoxelVolume(depth)
        assert volume.fillRandom(21, density) is volume
        want = model.random_set(21, model.threshold_of(density), S)
        assert np.array_equal(volume.download(), want), (S, density)
        assert want.sum() == {0.0: 0, 1.0: S ** 3}.get(density, want.sum())
        volume.close()
    for box in BOXES[S] + [(2, 2, 2, 2, 3, 3), (3, 3, 3, 1, 1, 1), (S, 0, 0, S + 4, 4, 4)]:      # the last three: empty, inverted, outside
        for op in (capi.VRC_COPY_REPLACE, capi.VRC_COPY_OR, capi.VRC_COPY_ANDNOT):
            for seed, threshold in [(5, 1 << 31), (0xFFFFFFFF, model.threshold_of(0.3)), (5, 0), (5, 1 << 32)]:
                volume = volume_of(base, depth)
                capi.check(capi.load().vrc_cells_fill_random(volume._h, seed, threshold, capi.ptr(np.array(box, np.uint32)), op, None))
                got, want = volume.download(), model.fill_random(base, seed, threshold, box, op)
                assert np.array_equal(got, want), (S, box, op, seed, threshold, differing(got, want))
                volume.close()


def test_fill_random_is_one_field_at_every_depth(built):
    import cpuvoxelraycaster_amd as vrc
    small, large = vrc.VoxelVolume(3), vrc.VoxelVolume(5)
    small.fillRandom(77, 0.37)
    large.fillRandom(77, 0.37)
    a, b = small.download(), large.download()
    assert 0 < a.sum() < 512 and np.array_equal(b[:8, :8, :8], a)
    # and in every box: two boxes that overlap fill their common voxels alike
    large.fillBoxes([[0, 0, 0, 32, 32, 32]], False)
    large.fillRandom(77, 0.37, (0, 0, 0, 20, 20, 20))
    large.fillRandom(77, 0.37, (11, 9, 7, 32, 32, 32))
    union = np.zeros((32, 32, 32), bool)
    union[:20, :20, :20] = True
    union[11:, 9:, 7:] = True
    assert np.array_equal(large.download(), b * union)
    with pytest.raises(vrc.VrcError):
        vrc.capi.check(vrc.capi.load().vrc_cells_fill_random(large._h, 1, (1 << 32) + 1, None, 1, None))
    with pytest.raises(ValueError):
        large.fillRandom(1, 1.5)
    small.close()
    large.close()


# ---- 9. the wrappers --------------------------------------------------------------------------------------------------

def test_smooth_remove_specks_and_caves(built):
    import cpuvoxelraycaster_amd as vrc
    for S in (8, 32):
        vol = model.three_band(S)
        for iterations, outside in [(1, False), (3, True)]:
            volume = volume_of(vol, depth_of(S))
            assert volume.smooth(iterations, outside) is volume
            assert np.array_equal(volume.download(), model.smooth(vol, iterations, int(outside))), (S, iterations, outside)
            volume.close()
        volume = volume_of(vol, depth_of(S))
        want = model.remove_specks(vol)
        assert volume.removeSpecks() is volume and np.array_equal(volume.download(), want) and want.sum() < vol.sum()
        assert volume.caves(1337, 0.48, 4) is volume
        assert np.array_equal(volume.download(), model.caves(S, 1337, 0.48, 4))
        volume.close()


def test_caves_commit_and_come_back(built):
    import cpuvoxelraycaster_amd as vrc
    S = 32
    want = model.caves(S, 1337, 0.48, 4)
    assert 0 < want.sum() < S ** 3
    volume = vrc.VoxelVolume(5).caves(1337, 0.48, 4)
    svo = volume.commit()
    back = vrc.VoxelVolume.fromScene(svo)
    assert np.array_equal(back.download(), want)
    for thing in (back, svo, volume):
        thing.close()
