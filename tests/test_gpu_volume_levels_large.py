"""The calls between depths where the launches of csrc/vrc_levels.hip stride: every kernel there is a grid-stride loop under
16384 workgroups, and no volume below 512^3 takes any of them into a second trip.  Here: cellCounts(4) at 512^3 (two trips of
k_counts_large) and, on ONE 1024^3 source made once for the module, cellCounts for k = 1 (eight trips of k_counts_bytes, the
512 MiB of counts compared on the device), 2 (four of k_counts_small<2>), 4 (sixteen of k_counts_large), 5 (two), 6 and 10 (on
the cap: one full pass, atomics); reduceInto 10 -> 8 (four trips of k_reduce_voxels<2>), 10 -> 6 (the sixteen trips into the
1 MiB scratch block and the kernel that reads it), 10 -> 5 and 10 -> 4; and expandInto depth 10 from depths 9 and 7 (eight trips
of k_expand).  The cases, their expected values and the trips they reach are tests/levels_cases.py's, held to their conditions
-- something in every trip, on both sides of every seam between trips, different in every trip -- and to levels_model.py in
tests/test_levels_cases_host.py.  Every expected value comes from a list of solid coordinates on the host, never from another
GPU result and never through an S^3 array; every comparison is exact.  A 1024^3 destination is held whole to its model by
solidCount() and the complete voxel list.  At most two 1024^3 volumes are alive at once.

Measured on the MI355X: the thirteen tests take 1.1 s together after the library's set-up, the slowest (512^3) 0.32 s, next to
1.55 s for the slowest test of test_gpu_volume_large.py in the same run; none skips."""
import functools

import numpy as np
import pytest

import cells_model
import levels_cases as cases
import levels_model as model

pytestmark = pytest.mark.gpu

REPLACE, OR, ANDNOT = cases.REPLACE, cases.OR, cases.ANDNOT


@functools.lru_cache(maxsize=None)
def garbage(depth, seed=5):
    """fillRandom(seed, 0.5)'s set, dense [x, y, z].  Shared: do not write to it."""
    vol = cells_model.random_set(seed, cells_model.threshold_of(0.5), 1 << depth)
    vol.setflags(write=False)
    return vol


def same(got, want, what):
    if not (got.shape == want.shape and np.array_equal(got, want)):
        where = np.argwhere(got != want) if got.shape == want.shape else []
        raise AssertionError("%s: shapes %s and %s, %d entries differ, the first at %s" % (what, got.shape, want.shape, len(where), where[:5].tolist() if len(where) else []))


def volume_with(c):
    import cpuvoxelraycaster_amd as vrc
    volume = cases.upload(vrc.VoxelVolume(c.depth), c)
    assert volume.solidCount() == len(c.solid)
    return volume


def check_reduce(src, solid, src_depth, dst_depth, ops):
    """into a destination full of fillRandom's voxels: "any" with REPLACE, then the splitting band under every op of `ops`"""
    import cpuvoxelraycaster_amd as vrc
    k = src_depth - dst_depth
    before = garbage(dst_depth)
    dst = vrc.VoxelVolume(dst_depth)
    bands = [(model.count_range("any", k), REPLACE)] + [(cases.split_band(solid, src_depth, k), op) for op in ops]
    for (lo, hi), op in bands:
        dst.fillRandom(5, 0.5, None, REPLACE)
        assert src.reduceInto(dst, lo, hi, op) is dst
        same(dst.download(), cases.reduce(before, solid, src_depth, lo, hi, op), ("reduce", src_depth, dst_depth, lo, hi, op))
    dst.close()


def check_whole_volume(volume, solid, what):
    """the volume holds exactly the voxels `solid` (a list without repetitions in any order): the count, then the whole list"""
    want = cases.in_list_order(solid, volume.depth)
    assert len(want) == len(solid)
    assert volume.solidCount() == len(want), (what, volume.solidCount(), len(want))
    got = volume.voxels()
    same(got.astype(np.int64), want, what)


# ---- 1. 512^3 ---------------------------------------------------------------------------------------------------------------

def test_counts_and_reduce_at_512(built):
    """cellCounts(4): two trips of k_counts_large, the seam at x = 256; k = 5 and 9 from the same volume in one pass; 9 -> 5
    through the same two trips into the scratch block, under the three ops"""
    c = cases.content(9)
    src = volume_with(c)
    for k in (4, 5, 9):
        got = src.cellCounts(k)
        same(got, cases.counts_dense(c.solid, 9, k), ("counts", 9, k))
        assert got.dtype == np.uint32 and np.array_equal(src.cellCounts(k), got)
    check_reduce(src, c.solid, 9, 5, (REPLACE, OR, ANDNOT))
    src.close()


# ---- 2. 1024^3, once ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def source(built):
    c = cases.content(10)
    volume = volume_with(c)
    yield volume, c.solid
    volume.close()


@pytest.mark.parametrize("k", [2, 4, 5, 6, 10])
def test_counts_at_1024(source, k):
    src, solid = source
    got = src.cellCounts(k)
    assert got.dtype == np.uint32
    same(got, cases.counts_dense(solid, 10, k), ("counts", 10, k))
    assert src.cellCounts(k).tobytes() == got.tobytes()                         # two calls, the same bytes: atomics from k = 6
    if k == 10:
        assert int(got[0, 0, 0]) == src.solidCount() == len(solid)


def test_counts_of_level_1_at_1024_stay_on_the_device(source):
    """2^27 counts, 512 MiB: compared on the device against zeros with the model's non-empty cells scattered in"""
    import torch
    src, solid = source
    cells, c = cases.counts_sparse(solid, 10, 1)
    want = torch.zeros(512 ** 3, dtype=torch.int32, device="cuda")
    want[torch.from_numpy(cells).cuda()] = torch.from_numpy(c.astype(np.int32)).cuda()
    got = src.cellCounts(1, device=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (512, 512, 512)
    if not torch.equal(got.reshape(-1), want):
        bad = torch.nonzero(got.reshape(-1) != want).reshape(-1)
        first = [(i >> 18, (i >> 9) & 511, i & 511) for i in bad[:5].cpu().tolist()]
        raise AssertionError("counts of level 1: %d cells differ, the first at %s" % (len(bad), first))
    del want
    assert torch.equal(src.cellCounts(1, device=True), got)


@pytest.mark.parametrize("dst_depth, ops", [(8, (REPLACE, OR, ANDNOT)), (6, (REPLACE, OR, ANDNOT)), (5, (REPLACE,)), (4, (REPLACE,))])
def test_reduce_from_1024(source, dst_depth, ops):
    src, solid = source
    check_reduce(src, solid, 10, dst_depth, ops)


def test_expand_512_into_a_solid_1024(built):
    """k = 1 with REPLACE into a destination that is solid throughout: everything outside the expected set is cleared"""
    import cpuvoxelraycaster_amd as vrc
    c = cases.content(9)
    src = volume_with(c)
    dst = vrc.VoxelVolume(10)
    dst.fillBoxes([[0, 0, 0, 1024, 1024, 1024]])
    assert dst.solidCount() == 1 << 30
    assert src.expandInto(dst) is dst
    check_whole_volume(dst, cases.expanded(c.solid, 1), "9 -> 10")
    dst.close()
    assert src.solidCount() == len(c.solid)
    src.close()


OR_BOXES = np.array([[100, 200, 300, 140, 210, 330],                             # by itself
                     [250, 0, 1000, 262, 8, 1024],                               # across the seam at x = 256
                     [500, 530, 10, 520, 560, 40]], np.uint32)                   # half inside the blown-up cube of the source


def test_expand_128_into_1024(built):
    """k = 3: OR into a destination that holds a few boxes, then REPLACE over the result"""
    import cpuvoxelraycaster_amd as vrc
    c = cases.content(7)
    src = volume_with(c)
    dst = vrc.VoxelVolume(10)
    dst.fillBoxes(OR_BOXES)
    blown = cases.expanded(c.solid, 3)
    in_boxes = np.concatenate([np.indices(tuple(b[3:].astype(np.int64) - b[:3])).reshape(3, -1).T + b[:3].astype(np.int64) for b in OR_BOXES])
    union = cases.in_list_order(np.concatenate([blown, in_boxes]), 10)
    assert len(blown) < len(union) < len(blown) + len(in_boxes)                  # the boxes add voxels, and one overlaps
    src.expandInto(dst, OR)
    check_whole_volume(dst, union, "7 -> 10, OR")
    src.expandInto(dst, REPLACE)
    check_whole_volume(dst, blown, "7 -> 10, REPLACE")
    dst.close()
    src.close()
