"""The calls between depths on the device (include/vrc.h: vrc_levels_counts, vrc_levels_reduce, vrc_levels_expand) against the
numpy model of levels_model.py, bit for bit after download().

The switches of csrc/vrc_levels.hip (vrc_levels.h), and the (source depth, k) pairs below that stand on either side of each:
  counts   k = 1 a lane per source word | k = 2, 3 a lane per cell | k = 4, 5 a workgroup per cell, stored | k >= 6 several
           workgroups per cell, atomics on zeroed counts: every depth 3 .. 7 runs every k up to the depth, so depth 4 has
           (1, 2, 3 | 4), depth 6 has (4, 5 | 6) and depth 7 has k = 7, 32 workgroups on one cell.
  reduce   k = 1 into 8^3 and more, a lane per word (4 -> 3, 5 -> 4, ...) | k = 1 into 4^3, a lane per voxel (3 -> 2);
           k = 2, 3 counted in the lane (4 -> 2, 5 -> 3, 5 -> 2, 6 -> 3, ...) | k >= 4 counts in the scratch block first
           (6 -> 2, 7 -> 3, 7 -> 2; 8 -> 2 is k = 6, where the scratch counts take atomics).
  dst      4^3 keeps two brick rows in a word: every source depth reduces down to depth 2.
No launch below 512^3 reaches the cap of 16384 workgroups, so no lane takes a second item at these sizes; the second and later
trips of every grid-stride loop run in test_gpu_volume_levels_large.py, at 512^3 and 1024^3 (the cases: levels_cases.py)."""
import functools

import numpy as np
import pytest

import cells_model
import levels_model as model
from volume_support import Stream, committed, expected_nodes, same, terrain_volume, volume_of

pytestmark = pytest.mark.gpu

REPLACE, OR, ANDNOT = model.REPLACE, model.OR, model.ANDNOT


@functools.lru_cache(maxsize=None)
def field(depth, seed=11, density=0.5):
    """fillRandom's set, dense [x, y, z].  Shared: do not write to it."""
    vol = cells_model.random_set(seed, cells_model.threshold_of(density), 1 << depth)
    vol.setflags(write=False)
    return vol


def random_volume(depth, seed=11, density=0.5):
    import cpuvoxelraycaster_amd as vrc
    return vrc.VoxelVolume(depth).fillRandom(seed, density, None, REPLACE)


def differing(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:4].tolist()


# ---- 1. every (source depth, k) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [3, 4, 5, 6, 7])
def test_every_level_of_a_random_field(built, depth):
    vol = field(depth)
    src = random_volume(depth)
    for k in range(1, depth + 1):
        want = model.counts(vol, k)
        got = src.cellCounts(k)
        assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), (depth, k, differing(got, want))
        assert np.array_equal(src.cellCounts(k), got)                          # two calls, the same bytes
    for dst_depth in range(depth - 1, 1, -1):
        k = depth - dst_depth
        dst = random_volume(dst_depth, seed=5)                                 # something to replace
        for rule in ("majority", (8 ** k // 2 + 1, 8 ** k + 1), "any", "all"):
            lo, hi = model.count_range(rule, k)
            assert src.reduceInto(dst, lo, hi) is dst
            got, want = dst.download(), model.reduced(vol, dst_depth, rule)
            assert np.array_equal(got, want), (depth, dst_depth, rule, differing(got, want))
        dst.close()
    assert np.array_equal(src.download(), vol)                                 # the source is only read
    src.close()


def test_depth_8_to_depth_2(built):
    """k = 6 through the scratch block: four workgroups add into every one of the 64 counts"""
    vol = field(8, seed=23)
    src = random_volume(8, seed=23)
    c = model.counts(vol, 6).astype(np.int64)
    lo = int(np.sort(c.reshape(-1))[32])                                       # a band that splits the 64 cells
    assert lo > 0 and 0 < (c >= lo).sum() < 64
    dst = random_volume(2, seed=5)
    for band in [(lo, 8 ** 6 + 1), (0, lo), (1, 8 ** 6 + 1)]:
        src.reduceInto(dst, *band)
        got, want = dst.download(), model.reduce(np.zeros((4, 4, 4), np.uint8), vol, *band)
        assert np.array_equal(got, want), (band, differing(got, want))
    assert np.array_equal(src.cellCounts(6), c) and src.cellCounts(8)[0, 0, 0] == vol.sum() == src.solidCount()
    src.close()
    dst.close()


# ---- 2. thresholds: cells that hold exactly the counts at the edges of the band -------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_thresholds(built, k):
    import cpuvoxelraycaster_amd as vrc
    full = 8 ** k
    lo, hi = full // 4 + 1, 3 * full // 4 - 1
    targets = [0, 1, lo - 1, lo, hi - 1, hi, full - 1, full]
    assert len(set(targets)) == 8
    rng = np.random.default_rng(40 + k)
    f, Sc = 1 << k, 8
    held = np.array(targets)[np.arange(Sc ** 3) % 8].reshape(Sc, Sc, Sc)
    rank = rng.permuted(np.tile(np.arange(full), (Sc ** 3, 1)), axis=1).reshape(Sc, Sc, Sc, f, f, f)
    vol = (rank < held[..., None, None, None]).transpose(0, 3, 1, 4, 2, 5).reshape(Sc * f, Sc * f, Sc * f).astype(np.uint8)
    assert np.array_equal(model.counts(vol, k), held)
    src, dst = volume_of(vol), vrc.VoxelVolume(3)
    assert np.array_equal(src.cellCounts(k), held)
    bands = [(lo, hi), (hi, lo), (lo, lo), (lo, 0xFFFFFFFF), (0, 0xFFFFFFFF), (full, 0xFFFFFFFF), (full + 1, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)]
    bands += [model.count_range(rule, k) for rule in model.RULES]
    for band in bands:
        dst.fillRandom(5, 0.5, None, REPLACE)
        src.reduceInto(dst, *band)
        want = ((held >= band[0]) & (held < band[1])).astype(np.uint8)
        got = dst.download()
        assert np.array_equal(got, want), (k, band, differing(got, want))
    for rule in model.RULES:
        made = src.reduced(3, rule)
        assert np.array_equal(made.download(), model.reduced(vol, 3, rule)), rule
        made.close()
    src.close()
    dst.close()


# ---- 3. corners: one voxel in each corner of the first, the last and an interior cell -------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_single_voxels_in_the_corners_of_a_cell(built, k):
    import cpuvoxelraycaster_amd as vrc
    f = 1 << k
    for dst_depth in (2, 3):
        Sc = 1 << dst_depth
        src, dst = vrc.VoxelVolume(dst_depth + k), vrc.VoxelVolume(dst_depth)
        for cell in [(0, 0, 0), (Sc - 1, Sc - 1, Sc - 1), (Sc // 2, Sc // 2 - 1, 1)]:
            for corner in range(8):
                voxel = [cell[a] * f + ((corner >> a) & 1) * (f - 1) for a in range(3)]
                src.setVoxels([voxel], True)
                want = np.zeros((Sc, Sc, Sc), np.uint32)
                want[cell] = 1
                got = src.cellCounts(k)
                assert np.array_equal(got, want), (k, dst_depth, voxel, np.argwhere(got).tolist())
                src.reduceInto(dst, 1, 8 ** k + 1)
                assert np.argwhere(dst.download()).tolist() == [list(cell)], (k, dst_depth, voxel)
                src.setVoxels([voxel], False)
        src.close()
        dst.close()


# ---- 4. the three ops over a destination that holds something ----------------------------------------------------------

@pytest.mark.parametrize("depth,dst_depth", [(3, 2), (4, 3), (5, 3), (6, 3), (6, 2), (7, 3)])
def test_reduce_ops_over_garbage(built, depth, dst_depth):
    vol, before = field(depth), field(dst_depth, seed=5)
    src, dst = random_volume(depth), random_volume(dst_depth, seed=5)
    lo, hi = model.count_range("majority", depth - dst_depth)
    for op in (REPLACE, OR, ANDNOT):
        dst.fillRandom(5, 0.5, None, REPLACE)
        src.reduceInto(dst, lo, hi, op)
        got, want = dst.download(), model.reduce(before, vol, lo, hi, op)
        assert np.array_equal(got, want), (op, differing(got, want))
    src.close()
    dst.close()


@pytest.mark.parametrize("depth,dst_depth", [(2, 3), (2, 5), (3, 4), (3, 6), (4, 7), (6, 7)])
def test_expand_ops_over_garbage(built, depth, dst_depth):
    vol, before = field(depth), field(dst_depth, seed=5)
    src, dst = random_volume(depth), random_volume(dst_depth, seed=5)
    for op in (REPLACE, OR, ANDNOT):
        dst.fillRandom(5, 0.5, None, REPLACE)
        assert src.expandInto(dst, op) is dst
        got, want = dst.download(), model.expand(before, vol, op)
        assert np.array_equal(got, want), (op, differing(got, want))
    assert np.array_equal(src.download(), vol)
    src.close()
    dst.close()


# ---- 5. expand is the affine stamp with the exact inverse map --------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3])
def test_expand_is_the_affine_stamp(built, k):
    import cpuvoxelraycaster_amd as vrc
    scale = 65536 >> k                                                         # q = ((2 p + 1) 2^(16 - k)) >> 17 = p >> k
    affine = vrc.make_affine([scale, 0, 0, 0, scale, 0, 0, 0, scale], [0, 0, 0])
    for depth in (2, 3, 4, 5):
        src = random_volume(depth, seed=31 + depth, density=0.4)
        stamped = src.transformed(affine, depth + k)
        blown = src.expanded(depth + k)
        got, want = blown.download(), stamped.download()
        assert np.array_equal(got, want), (k, depth, differing(got, want))
        assert np.array_equal(got, model.expand(np.zeros_like(got), field(depth, 31 + depth, 0.4)))
        for v in (src, stamped, blown):
            v.close()


# ---- 6. round trips ---------------------------------------------------------------------------------------------------

def test_round_trips(built):
    vol = field(3, seed=17)
    v = random_volume(3, seed=17)
    for k in (1, 2, 3, 4):
        big = v.expanded(3 + k)
        for rule in ("any", "all"):
            back = big.reduced(3, rule)
            assert np.array_equal(back.download(), vol), (k, rule)
            back.close()
        assert np.array_equal(big.cellCounts(k), vol.astype(np.uint32) * 8 ** k)
        big.close()
    v.close()
    w = random_volume(6, seed=18, density=0.3)
    solid = w.solidCount()
    assert solid == field(6, 18, 0.3).sum()
    for k in range(1, 7):
        assert int(w.cellCounts(k).astype(np.uint64).sum()) == solid, k
    assert w.cellCounts(6).shape == (1, 1, 1) and w.cellCounts(6)[0, 0, 0] == solid
    w.close()


@pytest.mark.parametrize("rule", ["any", "all"])
def test_levels_are_the_chain_of_single_levels(built, rule):
    """for "any" and "all" -- and for them only -- reducing level by level gives what reducing from the finest volume gives"""
    density = 0.002 if rule == "any" else 0.998                              # so that the levels down to 8^3 are neither full nor empty
    v = random_volume(6, seed=29, density=density)
    vol = field(6, 29, density)
    levels = v.levels(rule)
    assert [l.depth for l in levels] == [5, 4, 3, 2]
    step = v
    for level in levels:
        nxt = step.reduced(level.depth, rule)
        got, want = level.download(), model.reduced(vol, level.depth, rule)
        assert np.array_equal(got, want) and np.array_equal(nxt.download(), want), (rule, level.depth)
        assert 0 < want.sum() < want.size or level.depth == 2
        if step is not v:
            step.close()
        step = nxt
    step.close()
    for l in levels:
        l.close()
    v.close()


# ---- 7. memory and ordering -------------------------------------------------------------------------------------------

def test_counts_in_host_and_device_memory(built):
    import torch
    vol = field(6)
    src = random_volume(6)
    for k in range(1, 7):
        host = src.cellCounts(k)
        dev = src.cellCounts(k, device=True)
        assert dev.dtype == torch.int32 and tuple(dev.shape) == host.shape
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), host) and np.array_equal(host, model.counts(vol, k))
        # in place behind a 4-byte offset: the counts need no alignment beyond their own; the words around them stay
        n = host.size
        raw = torch.full((n + 2,), 0x55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with Stream() as stream:
            src.cellCountsDevice(k, raw.data_ptr() + 4, stream)
        out = raw.cpu().numpy().view(np.uint32)
        assert out[0] == 0x55 and out[-1] == 0x55 and np.array_equal(out[1:-1], host.reshape(-1)), k
    src.close()


@pytest.mark.parametrize("dst_depth", [5, 3, 2])
def test_reduce_sees_an_edit_in_flight(built, dst_depth):
    """a device-memory setVoxels on a stream, then the reduce on the same stream and on another one: both run behind it"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 64
    rng = np.random.default_rng(64)
    base = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
    extra = rng.integers(0, S, (200000, 3)).astype(np.uint32)
    edited = base.copy()
    edited[tuple(extra.T.astype(np.int64))] = 1
    lo, hi = model.count_range("majority", 6 - dst_depth)
    Sd = 1 << dst_depth
    want = model.reduce(np.zeros((Sd, Sd, Sd), np.uint8), edited, lo, hi)
    assert not np.array_equal(want, model.reduce(np.zeros((Sd, Sd, Sd), np.uint8), base, lo, hi))
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    torch.cuda.synchronize()
    for other_stream in (False, True):
        src, dst = volume_of(base, 6), vrc.VoxelVolume(dst_depth)
        with Stream() as stream, Stream() as second:
            src.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
            src.reduceInto(dst, lo, hi, REPLACE, second if other_stream else stream)
            got = dst.download()                                   # behind dst's last edit, the reduce
        assert np.array_equal(got, want), other_stream
        src.close()
        dst.close()


def edit_in_flight(S, seed, density=0.3):
    """(base, edited, the 200000 points between them as a device tensor): edited differs from base"""
    import torch
    rng = np.random.default_rng(seed)
    base = (rng.random((S, S, S)) < density).astype(np.uint8)
    extra = rng.integers(0, S, (200000, 3)).astype(np.uint32)
    edited = base.copy()
    edited[tuple(extra.T.astype(np.int64))] = 1
    assert not np.array_equal(base, edited)
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    torch.cuda.synchronize()
    return base, edited, t_extra


def test_counts_see_an_edit_in_flight(built):
    """the counts run behind src's last asynchronous edit, on its stream and on another one"""
    import torch
    base, edited, t_extra = edit_in_flight(64, 65)
    for k in (1, 3, 4):
        want = model.counts(edited, k)
        assert not np.array_equal(want, model.counts(base, k))
        for other_stream in (False, True):
            src = volume_of(base, 6)
            out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with Stream() as stream, Stream() as second:
                src.setVoxelsDevice(len(t_extra), t_extra.data_ptr(), True, stream)
                src.cellCountsDevice(k, out.data_ptr(), second if other_stream else stream)
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want), (k, other_stream, differing(got, want))
            src.close()


@pytest.mark.parametrize("edit_of", ["src", "dst"])
def test_expand_sees_an_edit_in_flight(built, edit_of):
    """64^3 into 128^3 behind a device-memory setVoxels on a stream -- of the source, and of the destination (OR, so that the
    destination's edit stays to be seen) -- on the same stream and on another one"""
    import cpuvoxelraycaster_amd as vrc
    src_vol = field(6, seed=41, density=0.3)
    if edit_of == "src":
        base, edited, t_extra = edit_in_flight(64, 66)
        want, op = model.expand(np.zeros((128, 128, 128), np.uint8), edited), REPLACE
        assert not np.array_equal(want, model.expand(np.zeros((128, 128, 128), np.uint8), base))
    else:
        base, edited, t_extra = edit_in_flight(128, 67, density=0.05)
        want, op = model.expand(edited, src_vol, OR), OR
        assert not np.array_equal(want, model.expand(base, src_vol, OR))
    for other_stream in (False, True):
        src = volume_of(base, 6) if edit_of == "src" else random_volume(6, seed=41, density=0.3)
        dst = vrc.VoxelVolume(7) if edit_of == "src" else volume_of(base, 7)
        with Stream() as stream, Stream() as second:
            (src if edit_of == "src" else dst).setVoxelsDevice(len(t_extra), t_extra.data_ptr(), True, stream)
            src.expandInto(dst, op, second if other_stream else stream)
            got = dst.download()                                   # behind dst's last edit, the expand
        assert np.array_equal(got, want), (edit_of, other_stream, differing(got, want))
        src.close()
        dst.close()


def test_reduced_volume_commits(built):
    vol = field(6, seed=37, density=0.45)
    src = random_volume(6, seed=37, density=0.45)
    for dst_depth, rule in [(5, "majority"), (4, "majority"), (3, "any")]:
        coarse = src.reduced(dst_depth, rule)
        want = model.reduced(vol, dst_depth, rule)
        assert 0 < want.sum() < want.size or rule == "any"
        assert same(committed(coarse), expected_nodes(want, dst_depth)), (dst_depth, rule)
        coarse.close()
    src.close()


# ---- 8. one large case: the 256^3 terrain ------------------------------------------------------------------------------

def test_terrain_256(built, heights):
    import cpuvoxelraycaster_amd as vrc
    vol = terrain_volume(heights, 8)
    src = vrc.VoxelVolume(8).raiseTerrain(heights)
    assert src.solidCount() == vol.sum()
    for dst_depth in (7, 4):
        k = 8 - dst_depth
        got, want = src.cellCounts(k), model.counts(vol, k)
        assert np.array_equal(got, want), (k, differing(got, want))
        for rule in ("any", "all", "majority"):
            coarse = src.reduced(dst_depth, rule)
            got, want = coarse.download(), model.reduced(vol, dst_depth, rule)
            assert np.array_equal(got, want), (dst_depth, rule, differing(got, want))
            coarse.close()
    src.close()


# ---- 9. the smallest sources: 4^3 is two words and one cell of level 2 ---------------------------------------------------

def test_depth_2_and_3_sources(built):
    import cpuvoxelraycaster_amd as vrc
    single = np.zeros((4, 4, 4), np.uint8)
    single[3, 2, 1] = 1
    for vol in (field(2), field(2, seed=3, density=0.8), np.ones((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), single):
        src = volume_of(vol, 2)
        for k in (1, 2):
            got, want = src.cellCounts(k), model.counts(vol, k)
            assert got.dtype == np.uint32 and got.shape == want.shape == (4 >> k,) * 3 and np.array_equal(got, want), (k, got.tolist(), want.tolist())
        assert int(src.cellCounts(2)[0, 0, 0]) == src.solidCount() == vol.sum()
        assert np.array_equal(src.download(), vol)
        src.close()
    for seed in (11, 12):
        vol = field(3, seed=seed)
        src = random_volume(3, seed=seed)
        got = src.cellCounts(3)
        assert got.shape == (1, 1, 1) and int(got[0, 0, 0]) == vol.sum() == src.solidCount()
        small = vrc.VoxelVolume(2)
        for rule in ("majority", "any", "all"):
            src.reduceInto(small, *model.count_range(rule, 1))
            assert np.array_equal(small.download(), model.reduced(vol, 2, rule)), (seed, rule)
        small.close()
        src.close()


# ---- 10. one destination for its whole life, under level differences that take the scratch block, leave it and come back ---

def test_one_destination_under_alternating_level_differences(built, heights):
    """into 4^3: k = 4 (counts stored), 6 (atomics on a block zeroed on the stream), 5 (stored), 6 again from other content,
    3 (no block); into 8^3 the same sources are k = 3, 5, 4, 5, 2.  A kernel that counted on finding the block clean, or on an
    earlier call's memset, leaves an earlier source's counts in the result.  vrc_volume_edit_scratch_bytes of neither volume
    moves"""
    import cpuvoxelraycaster_amd as vrc
    terrain = terrain_volume(heights, 8)
    sources = [(field(6), lambda: random_volume(6)), (field(8, seed=23), lambda: random_volume(8, seed=23)), (field(7), lambda: random_volume(7)),
               (terrain, lambda: vrc.VoxelVolume(8).raiseTerrain(heights)), (field(5), lambda: random_volume(5))]
    dsts = {2: vrc.VoxelVolume(2), 3: vrc.VoxelVolume(3)}
    scratch = {d: v.editScratchBytes() for d, v in dsts.items()}
    for step, (vol, make) in enumerate(sources):
        src = make()
        src_scratch = src.editScratchBytes()
        depth = vol.shape[0].bit_length() - 1
        for dst_depth, dst in dsts.items():
            k = depth - dst_depth
            c = np.sort(model.counts(vol, k).reshape(-1).astype(np.int64))
            lo = int(c[c > 0][(c > 0).sum() // 2])                             # a band that splits the cells
            assert 0 < (c >= lo).sum() < len(c)
            for band, op in (((lo, 8 ** k + 1), REPLACE), ((1, lo), OR), ((lo, 8 ** k + 1), ANDNOT)):
                before = dst.download()
                src.reduceInto(dst, *band, op)
                got, want = dst.download(), model.reduce(before, vol, *band, op)
                assert np.array_equal(got, want), (step, depth, dst_depth, band, op, differing(got, want))
            assert dst.editScratchBytes() == scratch[dst_depth], (step, dst_depth)
        assert np.array_equal(src.cellCounts(depth), [[[vol.sum()]]])
        assert src.editScratchBytes() == src_scratch, step
        src.close()
    for dst in dsts.values():
        dst.close()
