"""The cases of tests/test_gpu_volume_voxelize_large.py without a GPU (tests/voxelize_cases.py): the launch geometry restated
there puts the column scan on 2, 16, 32 and 64 lanes a brick column and on two words a lane, and the mark loop into its
second and later steps under split = 1, 1 < split < useful and the cap of 1024; the expected flips, which follow from how the
cases are made, are the model's (voxelize_model.column_flips), and that sparse form is the dense xor_mesh; and each of nine
wrong kernels, emulated, changes the result of the cases at every depth where it applies.  These are conditions on the
cases, not measurements of the kernels.  If the restated geometry stops matching the code, update the restatement; the
conditions stay."""
import numpy as np
import pytest

import large_volume_cases
import posed_cases
import voxelize_cases as cases
import voxelize_model as M

U = M.UNIT


# ---- the restated geometry --------------------------------------------------------------------------------------------

def test_restated_geometry():
    assert [cases.scan_geometry(d) for d in (3, 4, 5, 6, 7, 8, 9, 10)] == [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2)]
    assert [cases.n_words(d) for d in (3, 4, 9, 10)] == [16, 128, 1 << 22, 1 << 25]
    assert [cases.scan_groups(d) for d in (3, 4, 7, 9, 10)] == [1, 1, 256, 16384, 65536]
    for d in range(3, 11):                                                  # a column never straddles a wave, a lane's words never a column
        lanes, per = cases.scan_geometry(d)
        assert lanes * per == (1 << d) >> 3 and cases.WAVE % lanes == 0 and cases.scan_groups(d) * cases.GROUP * per >= cases.n_words(d)
    assert [cases.useful(d) for d in (2, 4, 5, 7, 9, 10)] == [1, 1, 4, 64, 1024, 4096]
    assert [cases.split(5, n) for n in (1, 1024, 4096, 4097, 4112)] == [4, 4, 1, 1, 1]
    assert [cases.split(7, n) for n in (1, 64, 65, 128, 150, 2000, 4096)] == [64, 64, 64, 32, 28, 3, 1]
    assert [cases.split(10, n) for n in (1, 4, 5)] == [1024, 1024, 820]
    assert [cases.stride_steps(i, l) for i, l in ((1, 256), (256, 256), (257, 256), (16384, 7168), (1 << 20, 1 << 18))] == [1, 1, 2, 3, 4]
    # the loop and its two wrong forms against the stride loop restated for the posed kernels
    for items, groups in ((1000, 1), (1000, 3), (5000, 4), (256, 2)):
        for loop, kw in (("stride", {}), ("once", dict(iterations=1)), ("group", dict(step_groups=1))):
            w = posed_cases.walk(items, groups, **kw)
            assert np.array_equal(np.bincount(w[:, 2], minlength=items), cases.visits(items, groups, loop)), (items, groups, loop)


def test_split_is_split_for_with_columns_for_words():
    """vrc_voxelize.hip:152-153: "the rule of split_for in vrc_volume.hip ... with columns for its words: keep the two in step".
    Both are split_rule -- the same 4096 and 1024 -- over their own units, and equal wherever neither unit binds"""
    same = 0
    for depth in range(2, 11):
        S = 1 << depth
        for n in list(range(1, 70)) + [127, 128, 129, 150, 1000, 2000, 4095, 4096, 4097, 20000, 1 << 20]:
            mine, theirs = cases.split(depth, n), large_volume_cases.split_for(depth, n)
            assert mine == cases.split_rule(n, S * S) and theirs == cases.split_rule(n, S ** 3 // 32), (depth, n)
            free = min((4096 + n - 1) // n, 1024)
            if free <= cases.useful(depth) and free <= (S ** 3 // 32 + 255) // 256:
                assert mine == theirs == free
                same += 1
    assert same > 200                                                       # of the 720 pairs tried


# ---- the scan cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", cases.SCAN_DEPTHS)
def test_scan_cases_reach_what_they_are_for(depth):
    case = cases.scan_case(depth)
    S, n = case.S, case.S >> 1
    lanes, per = cases.scan_geometry(depth)
    W = S >> 3
    # the expectation by construction is the model's, sparse; and dense where that is affordable
    assert np.array_equal(M.column_flips(S, case.tris), case.flips)
    if depth <= 8:
        assert np.array_equal(M.dense_of_flips(S, case.flips), M.xor_mesh(S, case.tris))
    borders = case.parts["borders"]
    # every word of a column is marked at its first and at its last nibble, the top word also from above the volume
    assert {int(k) for k in borders[:, 2]} >= {8 * j + 1 for j in range(W)} | {8 * j for j in range(1, W)} | {S, S + 3}
    assert len({(int(x), int(y)) for x, y, k in borders}) == len(borders)                # a column each: [0, k) is what comes out
    assert {(int(x) & 1, int(y) & 1) for x, y, k in borders} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    marks = cases.mark_words(depth, M.reduced(S, cases.mark_rows(depth, case.tris)))
    assert marks[0][0] == 0 and marks[0][-1] == cases.n_words(depth) - 1             # the first and the last word of the field
    bricks = (borders[:, 0] >> 1) * n + (borders[:, 1] >> 1)
    waves = bricks * W // per // cases.WAVE
    assert cases.scan_groups(depth) == 1 or len(np.unique(waves // 4)) >= 3               # several workgroups, where there are several
    if lanes < 64:
        assert len(np.unique(waves)) < len(np.unique(bricks))                           # brick columns that share a wave
    # crossings: two marks in one column, in different lanes; at depth 10 also in one lane's two words
    cross = case.parts["crossings"].reshape(-1, 2, 3)
    lane_of = (cross[:, :, 2] - 1) // 8 // per
    assert (cross[:, 0, :2] == cross[:, 1, :2]).all() and (lane_of[:, 0] != lane_of[:, 1]).sum() >= 3
    if per == 2:
        word_of = (cross[:, :, 2] - 1) // 8
        assert ((lane_of[:, 0] == lane_of[:, 1]) & (word_of[:, 0] != word_of[:, 1])).sum() >= 3
    # neighbours: the unmarked column of each pair stays empty, as do the marked brick's other three voxel columns
    flip_bricks = (case.flips[:, 0] >> 1) * n + (case.flips[:, 1] >> 1)
    assert not np.isin(flip_bricks, case.empty_bricks).any()
    for x, y in {(int(x), int(y)) for x, y, k in case.parts["neighbours"]}:
        inside = (case.flips[:, 0] >> 1 == x >> 1) & (case.flips[:, 1] >> 1 == y >> 1)
        assert inside.any() and ((case.flips[inside, 0] == x) & (case.flips[inside, 1] == y)).all()
    # words whose marks cancel: toggled, and no mark left in them
    toggled = cases.mark_words(depth, case.parts["cancelled"][:2])[0]
    assert len(toggled) == 2 and not np.isin(toggled, marks[0]).any()
    # the layer: exact repeats, which cancel, and several marks in one word
    layer = case.parts["layer"]
    assert len(layer) == 300 and len(np.unique(layer, axis=0)) < 290
    left = cases.mark_words(depth, M.reduced(S, layer))
    assert max(bin(int(b)).count("1") for b in left[1]) >= 2
    # the emulated scan of the marks is the expectation, word for word
    got, want = cases.scan(depth, marks), cases.flip_words(depth, case.flips)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert cases.popcount(want[1]) == M.count_of_flips(case.flips)
    # into a non-empty volume: the boxes do not overlap, meet touched columns and lie elsewhere too
    boxes = cases.before_boxes(depth)
    runs = M.runs_of_flips(case.flips)
    inside = cases.solid_in_boxes(boxes, runs)
    assert 0 < inside < M.count_of_flips(case.flips) and inside < cases.boxes_volume(boxes)
    if depth <= 7:
        dense = cases.dense_boxes(S, boxes)
        assert int(dense.sum()) == cases.boxes_volume(boxes)
        assert int((dense & M.dense_of_flips(S, case.flips)).sum()) == inside


# ---- the stride cases -------------------------------------------------------------------------------------------------

STEPS = {(5, None): (4112, 1, 4, False), (7, 128): (128, 32, 2, False), (7, 150): (150, 28, 3, True), (9, None): (8, 512, 2, False),
         (10, None): (4, 1024, 4, False)}                    # n, split, steps of a slab's triangle, is the last step partial


@pytest.mark.parametrize("depth, n", cases.STRIDE_CASES)
def test_stride_cases_take_the_steps_they_claim(depth, n):
    case = cases.stride_case(depth, n)
    S = case.S
    count, split, steps, partial = STEPS[depth, n]
    assert len(case.tris) == case.n == count and cases.split(depth, count) == split
    assert (split == 1) == (depth == 5) and (depth != 7 or 1 < split < cases.useful(7)) and (depth != 10 or split == 1024 < cases.useful(10))
    lanes = cases.lanes_per_triangle(depth, count)
    for t in case.slabs:
        items = cases.triangle_items(S, t)
        assert items == S * S and cases.stride_steps(items, lanes) == steps >= 2 and (items % lanes != 0) == partial
    where = [i for i, t in enumerate(case.tris) if cases.triangle_items(S, t) == S * S]
    assert len(where) == len(case.slabs) and (depth != 5 or (where[0] == 0 and where[-1] == count - 1 and any(2000 < i < 2100 for i in where)))
    # the slabs by construction are the model's, and the whole expectation is the model's where the model is affordable
    assert np.array_equal(M.column_flips(S, case.slabs), M.reduced(S, case.slab_rows))
    if depth <= 9:
        assert np.array_equal(M.column_flips(S, case.tris), case.flips)
    if depth <= 7:
        assert np.array_equal(M.dense_of_flips(S, case.flips), M.xor_mesh(S, case.tris))
    k = case.slab_rows[:, 2]
    assert (k == S).any() and (k < S).any() and 0 < M.count_of_flips(case.flips)           # clamped at the top in a corner


def test_depth_10_slab_in_python_integers():
    """the largest products of the rule: a sample of columns rechecked in Python integers, and the bound they reach"""
    case = cases.stride_case(10)
    S = case.S
    assert np.abs(case.tris.reshape(-1, 3, 3)[:, :, :2]).max() == M.LIMIT and np.abs(case.tris).max() == M.LIMIT
    rng = np.random.default_rng(10)
    sample = [(0, 0), (1023, 1023), (0, 1023), (1023, 0), (511, 512)] + rng.integers(0, S, (300, 2)).tolist()
    largest = 0
    rows = []
    for x, y in sample:
        for t in case.tris:
            got = M.column_exact(S, t, x, y)
            if got is not None:
                rows.append((x, y, got[0]))
                largest = max(largest, got[1])
    rows = M.reduced(S, np.array(rows))
    key = lambda r: (r[:, 0] * S + r[:, 1])
    mine = case.flips[np.isin(key(case.flips), key(np.array(sample)))]
    assert np.array_equal(rows, mine) and len(rows) > 400
    print("depth-10 slab: |N| + D reaches 2^%.2f" % np.log2(float(largest)))
    assert 1 << 52 < largest < 1 << 57


def test_the_existing_gpu_tests_take_one_step_but_for_one():
    """Every (depth, triangles) that tests/test_gpu_volume_voxelize.py voxelises, with the widest clipped bounding box of its
    triangles against the lanes its launch gives a triangle.  All but one stay within one step of the mark loop.  The one:
    test_algebra's icosphere and spanning tetrahedron in one call (324 triangles at 64^3: 13 workgroups, 3328 lanes, for
    4096 columns) takes a second step -- and is the one call whose result that file compares with other device results
    only (order, winding, twice = never, terrain ^ once), never with the model."""
    import test_gpu_volume_voxelize as G
    import test_volume_voxelize_host as H
    calls = []
    for depth in (2, 3, 5, 6):
        S = 1 << depth
        rng = np.random.default_rng(100 + depth)
        calls.append(("tetrahedron", depth, G.tetrahedron(S, rng)))
        calls.append(("icosphere", depth, G.sphere(S, 0.7 * S, (S / 2 + 0.3, S / 2 - 0.2, S / 2 + 0.1))))
        for i in range(3):
            v = rng.integers(-S * U // 2, 3 * S * U // 2, (4, 3))
            calls.append(("random tetrahedron", depth, M.soup(v, [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)])))
        for lo, hi in (((1, 0, 1), (S - 1, S // 2, S)), ((0, 0, 0), (S, S, S)), ((S // 4, 1, S // 2 - 1), (S // 4 + 1, 3, S // 2 + 1))):
            calls.append(("box", depth, G.box(lo, hi)))
    calls.append(("half-voxel box", 5, G.box((2.5, 3.5, 1.5), (10.5, 8.5, 29.5))))
    calls += [("fan", depth, H.fan(5 * U)) for depth in (2, 3, 5)]
    calls.append(("borders under a roof", 6, np.concatenate([G.sheet(20, 20, 21, 21, U)] * 8 + [G.sheet(19, 19, 25, 23, 70 * U)])))
    calls.append(("cancelling sheets", 5, np.concatenate([G.sheet(3, 4, 9, 11, 5 * U + 3), G.sheet(5, 2, 12, 8, 5 * U + 20), G.sheet(0, 0, 7, 7, 17 * U)])))
    calls.append(("degenerate and roof", 5, np.concatenate([np.zeros((4, 9), np.int32), G.sheet(2, 2, 20, 20, 9 * U + 5), np.zeros((4, 9), np.int32)])))
    calls.append(("memory kinds", 6, G.sphere(64, 25.2, (31.3, 33.1, 28.8))))
    calls.append(("ordered", 6, G.sphere(64, 22.6, (30.2, 29.7, 31.4))))
    rng = np.random.default_rng(20)
    calls.append(("scratch: small icosphere", 6, G.sphere(64, 40, (32, 32, 32), 1)))
    calls.append(("scratch: tetrahedron", 6, G.tetrahedron(64, rng)))
    calls.append(("scratch: roof", 6, G.sheet(-3, 5, 50, 70, 37 * U + 11)))
    calls.append(("many small items", 6, cases.tetrahedra(64, 5000, np.random.default_rng(5))))
    calls.append(("spanning box", 6, G.box((0, 0, 0), (64, 64, 64))))
    calls.append(("spanning box off the grid", 6, G.box((-5.5, -1, 0.5), (64 + 3, 64 - 0.5, 64 - 1.5))))
    calls.append(("stamp clipboard", 5, G.sphere(32, 14.6, (15.3, 14.9, 15.2))))
    calls.append(("no holes", 6, G.sphere(64, 24.3, (31.7, 32.2, 30.9), 3)))
    rng = np.random.default_rng(3)
    algebra = np.concatenate([G.sphere(64, 19.4, (30.1, 27.9, 33.3)), G.tetrahedron(64, rng)])
    second = []
    for name, depth, tris in calls + [("algebra", 6, algebra), ("algebra: the ball alone", 6, G.sphere(64, 11.7, (20.3, 22.8, 19.6)))]:
        widest = max(cases.triangle_items(1 << depth, t) for t in tris)
        lanes = cases.lanes_per_triangle(depth, len(tris))
        print("%-28s depth %d  n %5d  widest %5d columns  lanes %5d" % (name, depth, len(tris), widest, lanes))
        if cases.stride_steps(max(widest, 1), lanes) > 1:
            second.append((name, len(tris), widest, lanes))
    assert second == [("algebra", 324, 4096, 3328)], second


# ---- the sparse form of the model -------------------------------------------------------------------------------------

def test_sparse_model_is_the_dense_model():
    """column_flips -> dense_of_flips is xor_mesh on the existing host cases: the fan in its eight copies, the half-voxel box,
    random tetrahedra partly outside, degenerate and out-of-range triangles; into a non-empty field; runs and counts"""
    import test_volume_voxelize_host as H
    rng = np.random.default_rng(7)
    lists = [(16, H.fan(h, mx, my, sw)) for mx, my, sw in H.FAN_VARIANTS for h in (5 * U, 5 * U + 32, 5 * U + 33, 32, 33, 40 * U, -U)]
    lists.append((32, H.box_tris((2.5, 3.5, 1.5), (10.5, 8.5, 29.5))))
    lists.append((16, H.box_tris((-3, 5, -2), (4, 20, 7))))
    for S in (4, 16, 64):
        for _ in range(6):
            v = rng.integers(-S * U // 2, 3 * S * U // 2, (4, 3))
            lists.append((S, M.soup(v, [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)])))
    far = np.array([[0, 0, 200, (1 << 17) + 1, 0, 200, 0, 512, 200], [0, 0, 0, 512, 0, 0, 512, 0, 512], [0, 0, 200, 1 << 17, 0, 200, 0, 512, 200]], np.int32)
    lists.append((8, far))
    lists.append((32, np.concatenate([t for S, t in lists if S == 16][:20])))            # many lists in one: crossings cancel
    for S, tris in lists:
        dense = M.xor_mesh(S, tris)
        flips = M.column_flips(S, tris)
        assert np.array_equal(M.dense_of_flips(S, flips), dense)
        assert M.count_of_flips(flips) == int(dense.sum())
        runs = M.runs_of_flips(flips)
        again = np.zeros_like(dense)
        for x, y, z0, z1 in runs.tolist():
            assert z0 < z1 and not again[x, y, z0:z1].any()
            again[x, y, z0:z1] = 1
        assert np.array_equal(again, dense)
        before = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
        assert np.array_equal(M.dense_of_flips(S, flips, before.copy()), M.xor_mesh(S, tris, before.copy()))
        depth = S.bit_length() - 1
        if depth >= 3:
            import delta_model
            rec, _ = delta_model.diff(delta_model.words_of(np.zeros_like(dense)), delta_model.words_of(dense), depth)
            words, bits = cases.flip_words(depth, flips)
            assert np.array_equal(words, rec["word"]) and np.array_equal(bits, rec["bits"])


def test_stamped_icosphere_needs_a_depth_8_clipboard():
    from cpuvoxelraycaster_amd import scenes
    verts, faces = scenes.icosphere(cases.STAMP["subdivisions"])
    fixed = M.quantise(verts, cases.STAMP["radius"], cases.STAMP["centre"]).astype(np.int64)
    lo = fixed.min(axis=0) >> 6
    size = -((-fixed.max(axis=0)) >> 6) - lo
    assert 128 < size.max() <= 256 and size.min() >= 150 and (lo % 2 == 1).any() and lo.min() > 0 and (lo + size).max() < 256
    flips = cases.stamp_flips(verts, faces)
    assert 1500000 < M.count_of_flips(flips) < 4 / 3 * np.pi * cases.STAMP["radius"] ** 3


# ---- each wrong kernel changes the result -----------------------------------------------------------------------------

# voxels of the scan cases' result that a wrong scan changes, per depth; None: the switch does not apply there (one word a
# lane has no order, no handing down and one word to take `own` from).  The guard matters at 64 lanes too: no other column
# is there to leak in, but a lane whose source lies beyond the wave reads its own value and would cancel itself
WRONG_SCAN = {
    "no_guard":     {4: 128, 7: 9664, 8: 21408, 9: 31992, 10: 87136},
    "stop_early":   {4: 136, 7: 4400, 8: 8744, 9: 22200, 10: 61584},
    "wrong_pos":    {4: 72, 7: 5632, 8: 14776, 9: 35672, 10: 109552},
    "ascending":    {4: None, 7: None, 8: None, 9: None, 10: 4056},
    "no_handoff":   {4: None, 7: None, 8: None, 9: None, 10: 2128},
    "own_one_word": {4: None, 7: None, 8: None, 9: None, 10: 107488},
}
NO_CLAMP_SCAN = {4: 19, 7: 131, 8: 259, 9: 515, 10: 1027}
# voxels of the stride cases' result that a wrong mark loop changes; "group" (it += blockDim.x) is the right loop at split = 1
WRONG_MARK = {
    (5, None): dict(once=1910, group=None, no_clamp=3844),
    (7, 128): dict(once=23136, group=32784, no_clamp=30738),
    (7, 150): dict(once=25392, group=33908, no_clamp=30738),
    (9, None): dict(once=508746, group=827426),
    (10, None): dict(once=2167571, group=2560787),
}


@pytest.mark.parametrize("depth", cases.SCAN_DEPTHS)
def test_each_wrong_scan_changes_the_scan_cases(depth):
    case = cases.scan_case(depth)
    lanes, per = cases.scan_geometry(depth)
    for wrong in cases.SCAN_SWITCHES:
        applies = wrong in ("no_guard", "stop_early", "wrong_pos") or per == 2
        changed = cases.voxels_changed(depth, case.tris, wrong)
        print("depth %d %s: %d voxels change" % (depth, wrong, changed))
        assert changed == (WRONG_SCAN[wrong][depth] or 0), (wrong, depth, changed)
        assert (changed > 0) == applies, (wrong, depth)
    changed = cases.voxels_changed(depth, case.tris, "no_clamp")
    assert changed == NO_CLAMP_SCAN[depth] > 0


@pytest.mark.parametrize("depth, n", cases.STRIDE_CASES)
def test_each_wrong_mark_loop_changes_the_stride_cases(depth, n):
    case = cases.stride_case(depth, n)
    for wrong, want in WRONG_MARK[depth, n].items():
        changed = cases.voxels_changed(depth, case.tris, wrong)
        print("depth %d n %d %s: %d voxels change" % (depth, case.n, wrong, changed))
        assert changed == (want or 0), (wrong, depth, changed)
        assert (changed > 0) == (wrong != "group" or cases.split(depth, case.n) > 1)
