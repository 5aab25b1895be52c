"""The cases of tests/test_gpu_volume_levels_large.py without a GPU (tests/levels_cases.py): the launch geometry restated
there gives the trips that csrc/vrc_levels.hip takes at 512^3 and 1024^3; the maps between items and voxels are each other's
inverse and tile the volume; the models on a list of solid voxels are levels_model.py's on small dense volumes; and the
content puts something that matters into every trip, onto both sides of every seam between two trips, and differently
into every trip.  If the restated geometry stops matching the code, update the restatement; the conditions stay."""
import numpy as np
import pytest

import levels_cases as cases
import levels_model as model

ALL_OPS = (cases.REPLACE, cases.OR, cases.ANDNOT)


# ---- the launch geometry --------------------------------------------------------------------------------------------------

# (kind, source depth, k): kernel, items, trips, the pitch of the trip seams along the SOURCE's x (expand: the destination's)
STRIDING = [
    ("counts", 9, 4, "k_counts_large", 1 << 15, 2, 256),
    ("reduce", 9, 4, "k_counts_large", 1 << 15, 2, 256),
    ("counts", 10, 4, "k_counts_large", 1 << 18, 16, 64),
    ("reduce", 10, 4, "k_counts_large", 1 << 18, 16, 64),
    ("counts", 10, 5, "k_counts_large", 1 << 15, 2, 512),
    ("reduce", 10, 5, "k_counts_large", 1 << 15, 2, 512),
    ("counts", 10, 1, "k_counts_bytes", 1 << 25, 8, 128),
    ("counts", 10, 2, "k_counts_small<2>", 1 << 24, 4, 256),
    ("reduce", 10, 2, "k_reduce_voxels<2>", 1 << 24, 4, 256),
    ("expand", 9, 1, "k_expand", 1 << 25, 8, 128),
    ("expand", 7, 3, "k_expand", 1 << 25, 8, 128),
]


def test_the_launches_that_stride():
    assert cases.MAX_GROUPS * cases.GROUP == 1 << 22
    for kind, depth, k, kernel, items, trips, pitch in STRIDING:
        launch = cases.striding(kind, depth, k)
        per_pass = cases.MAX_GROUPS if kernel == "k_counts_large" else cases.MAX_GROUPS * cases.GROUP
        assert launch.row() == (kernel, items, per_pass, trips), (kind, depth, k, launch.row())
        lo, hi = launch.cover(np.array(launch.seams(), np.int64))
        scale = k if kernel.startswith("k_reduce") else 0                      # a destination voxel of reduce is a cell of the source
        size = 1024 if kind == "expand" else 1 << depth
        assert (lo[:, 0] << scale).tolist() == list(range(pitch, size, pitch)), (kind, depth, k)
        assert not lo[:, 1:].any()                                             # a trip begins with a whole plane of x
    # every call of the GPU tests has its row, and the table of the summary is made of them
    assert {c for c in cases.CASES if cases.striding(*c).trips > 1} == {row[:3] for row in STRIDING}
    assert len(cases.trip_table()) == len(cases.CASES) + 4                     # reduce with k >= 4 is two launches


def test_the_launches_that_do_not_stride():
    one_pass = lambda kind, depth, k: [l.trips for l in cases.launches(kind, depth, k)]
    for depth in range(3, 11):
        assert one_pass("reduce", depth, 1) == [1]                             # k_reduce_bytes (3 -> 2: k_reduce_voxels<1>)
        for k in range(1, depth + 1):
            strides = any(t > 1 for t in one_pass("counts", depth, k))
            assert strides == ((depth, k) in [(9, 4), (10, 1), (10, 2), (10, 4), (10, 5)]), (depth, k)
        for k in range(1, depth - 1):
            voxels = cases.launches("reduce", depth, k)[-1]
            assert (voxels.trips > 1) == ((depth, k) == (10, 2)), (depth, k)
    assert cases.launches("reduce", 10, 1)[0].row() == ("k_reduce_bytes", 1 << 22, 1 << 22, 1)
    assert cases.launches("counts", 10, 3)[0].row() == ("k_counts_small<3>", 1 << 21, 1 << 21, 1)
    assert cases.launches("reduce", 10, 3)[0].row() == ("k_reduce_voxels<3>", 1 << 21, 1 << 21, 1)
    assert cases.launches("reduce", 10, 4)[1].row() == ("k_reduce_voxels<0>", 1 << 18, 1 << 18, 1)
    for k in (6, 7, 8, 9, 10):                                                 # on the cap: one full pass
        assert cases.launches("counts", 10, k)[0].row() == ("k_counts_large", 16384, 16384, 1), k
    for src in range(2, 9):
        for k in range(1, 10 - src):
            assert cases.launches("expand", src, k)[0].trips == 1
    assert [cases.groups_for(n) for n in (1, 256, 257, (1 << 22) - 1, 1 << 22, (1 << 22) + 1)] == [1, 1, 2, 16384, 16384, 16384]


@pytest.mark.parametrize("kind, depth, k", [("counts", 6, 1), ("counts", 6, 2), ("counts", 5, 3), ("counts", 6, 4), ("counts", 6, 5),
                                            ("counts", 6, 6), ("counts", 8, 8), ("reduce", 4, 1), ("reduce", 3, 1), ("reduce", 5, 2),
                                            ("reduce", 4, 2), ("reduce", 6, 4), ("expand", 2, 3), ("expand", 4, 1)])
def test_items_and_voxels_are_each_others(kind, depth, k):
    """every launch of the call: the boxes of all items tile the volume they cover, and item_of gives every voxel of a box
    its item"""
    for launch in cases.launches(kind, depth, k):
        S = 1 << launch.depth
        items = np.arange(launch.items, dtype=np.int64)
        lo, hi = launch.cover(items)
        assert (lo >= 0).all() and (hi <= S).all() and (hi > lo).all()
        assert int((hi - lo).prod(axis=1).sum()) == S ** 3, launch.kernel
        if S <= 64:
            p = np.indices((S, S, S)).reshape(3, -1).T
            of = launch.item_of(p)
            assert ((p >= lo[of]) & (p < hi[of])).all(), launch.kernel
        else:
            assert np.array_equal(launch.item_of(lo), items) and np.array_equal(launch.item_of(hi - 1), items), launch.kernel


def test_a_part_is_group_words_of_a_cell():
    """k_counts_large from k = 6: a unit's box holds LEVELS_GROUP_WORDS words of 32 voxels"""
    for k in (6, 7, 8, 9, 10):
        launch = cases.counts_launch(10, k)
        lo, hi = launch.cover(np.arange(launch.items, dtype=np.int64))
        assert ((hi - lo).prod(axis=1) == cases.LEVELS_GROUP_WORDS * 32).all(), k
    for k in (4, 5):
        lo, hi = cases.counts_launch(10, k).cover(np.arange(8, dtype=np.int64))
        assert ((hi - lo) == 1 << k).all()


# ---- the models on a list ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [4, 5, 6])
def test_the_list_models_are_levels_model(depth):
    S = 1 << depth
    rng = np.random.default_rng(300 + depth)
    vol = (rng.random((S, S, S)) < 0.4).astype(np.uint8)
    vol[:8, 8:16, :8] = 1                                                      # full cells up to k = 3
    solid = rng.permutation(np.argwhere(vol))                                  # in no order
    assert np.array_equal(cases.dense_of(solid, depth), vol)
    for k in range(1, depth + 1):
        want = model.counts(vol, k)
        got = cases.counts_dense(solid, depth, k)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), k
        cells, c = cases.counts_sparse(solid, depth, k)
        assert np.array_equal(cells, np.flatnonzero(want)) and np.array_equal(c, want.reshape(-1)[cells])
    for dst_depth in range(2, depth):
        k = depth - dst_depth
        before = (rng.random((1 << dst_depth,) * 3) < 0.5).astype(np.uint8)
        bands = [model.count_range(rule, k) for rule in model.RULES] + [cases.split_band(solid, depth, k), (3, 3), (2, 8 ** k // 3)]
        for lo, hi in bands:
            for op in ALL_OPS:
                assert np.array_equal(cases.reduce(before, solid, depth, lo, hi, op), model.reduce(before, vol, lo, hi, op)), (k, lo, hi, op)
            if lo >= 1:
                K = model.reduce(np.zeros_like(before), vol, lo, hi)
                assert np.array_equal(cases.dense_of(cases.selected(solid, depth, k, lo, hi), dst_depth), K), (k, lo, hi)
    for k in range(1, 8 - depth):
        big = cases.expanded(solid, k)
        assert len(np.unique(cases.list_key(big, depth + k))) == len(big) == len(solid) * 8 ** k
        assert np.array_equal(cases.dense_of(big, depth + k), model.expand(np.zeros((S << k,) * 3, np.uint8), vol)), k


def test_list_order_is_the_voxel_lists():
    """list_key against the order written out: bricks by (x, y, z), inside a brick z, y, x from the slowest"""
    depth, S = 3, 8
    p = np.indices((S, S, S)).reshape(3, -1).T
    by_hand = sorted(map(tuple, p.tolist()), key=lambda v: (v[0] >> 1, v[1] >> 1, v[2] >> 1, v[2] & 1, v[1] & 1, v[0] & 1))
    twice = np.concatenate([p[::-1], p[::3]])
    assert cases.in_list_order(twice, depth).tolist() == [list(v) for v in by_hand]
    assert cases.list_key(np.array([[7, 7, 7]]), depth)[0] == S ** 3 - 1


# ---- the content ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [7, 9, 10])
def test_content(depth):
    c = cases.content(depth)
    S = 1 << depth
    pitch = cases.CONTENT[depth][0]
    assert c.solid.min() == 0 and c.solid.max() == S - 1 and (np.diff(cases.list_key(c.solid, depth)) > 0).all()
    in_boxes = sum(int(np.prod(b[3:].astype(np.int64) - b[:3])) for b in c.boxes)
    print("depth %d: %d points and %d boxes to upload, %d solid voxels" % (depth, len(c.points), len(c.boxes), len(c.solid)))
    assert len(c.solid) > in_boxes and len(c.solid) <= len(c.points) + in_boxes < 600000
    have = set(map(tuple, c.solid.tolist()))
    assert (0, 0, 0) in have and (S - 1,) * 3 in have
    for s in range(pitch, S, pitch):
        assert (s, 0, 0) in have and (s - 1, S - 1, S - 1) in have
        for x in (s - 2, s - 1, s, s + 1):
            assert int((c.solid[:, 0] == x).sum()) > 10, (s, x)
    assert cases.content(depth) is c                                          # made once


def check_items(what, launch, items, values=None, seams=True):
    facts = cases.item_facts(launch, items, values)
    assert facts["trips"] == list(range(launch.trips)), (what, facts["trips"])
    assert facts["distinct"] or launch.trips == 1, what
    if seams:
        assert facts["first"] and facts["last"], what
        assert facts["seams"] == launch.seams(), (what, facts["seams"])
    return facts


@pytest.mark.parametrize("kind, depth, k", cases.CASES)
def test_every_case_meets_its_trips(kind, depth, k):
    """the conditions of every call of the GPU tests on the launch of it that strides (one pass where none does: then the
    first and the last item and one trip).  A reduce is held to them under "any" and, but for the items at the seams, under
    its splitting band; with k >= 4 its striding launch is the counts', whose outputs do not depend on the band"""
    launch, items, values = cases.nonzero_items(kind, depth, k)
    solid = cases.content(depth).solid
    what = (kind, depth, k, launch.kernel)
    check_items(what, launch, items, values)
    print("%s depth %d k %d: %s, %d items a pass of %d, %d trips, %d items with output" % (kind, depth, k, *launch.row(), len(items)))
    if kind == "counts":
        if 2 <= k <= 5:                                                        # an item is a cell, and a cube fills some
            assert (values == 8 ** k).any() and (values < 8 ** k).any(), what
        return
    if kind == "expand":
        assert len(cases.expanded(solid, k)) < 1 << 20                         # one window of the voxel list
        return
    band = cases.split_band(solid, depth, k)
    cells, c = cases.counts_sparse(solid, depth, k)
    chosen = cells[(c >= band[0]) & (c < band[1])]
    print("    band %s selects %d of %d non-empty cells of %d" % (band, len(chosen), len(cells), 8 ** (depth - k)))
    assert 0 < len(chosen) < len(cells)
    if k < 4:
        _, split_items, _ = cases.nonzero_items(kind, depth, k, band)
        check_items(what + band, launch, split_items, seams=False)
    else:                                                                      # the trips of the counts that hold a selected cell
        lgp = max(3 * k - 16, 0)
        for some in (chosen, np.setdiff1d(cells, chosen)):
            trips = np.unique((some << lgp) // launch.per_pass)
            assert len(trips) >= min(launch.trips, 8), (what, trips.tolist())


def test_a_wrong_stride_would_show():
    """what the conditions are for, on the 16 trips of 10 -> 6: counts that stop after one trip, that read trip 0's cells in
    every trip, or that skip the item on one side of a seam differ from the expected counts in every trip"""
    launch, items, values = cases.nonzero_items("reduce", 10, 4)
    want = np.zeros(launch.items, np.int64)
    want[items] = values
    by_trip = want.reshape(launch.trips, launch.per_pass)
    assert (by_trip[1:].sum(axis=1) > 0).all()                                 # one trip only: every later trip stays zero
    assert all((by_trip[t] != by_trip[0]).any() for t in range(1, launch.trips))
    assert (by_trip[:, 0] > 0).all() and (by_trip[:, -1] > 0).all()
