"""The cases of tests/test_gpu_volume_posed_large.py without a GPU (tests/posed_cases.py): the scene is what it claims, the
launch geometry restated there puts the posed kernels of vrc_rigid.hip into the regime the GPU tests are meant for -- a lane
that adds posed voxels in several iterations of its stride loop, a broad phase with a second workgroup -- and the records
computed from voxel lists are the models' own.  If the restated geometry stops matching the code, update the restatement;
the conditions stay."""
import numpy as np

import contact_model
import pair_contact_model
import posed_cases as cases
import rigid_model
import stamp_model

S = 128
WHOLE = [0, 0, 0, S, S, S]


def test_scene_is_a_frame_and_256_blocks():
    case = cases.large_case()
    rec = case.rec
    assert len(rec) == 257
    assert int(case.vol.sum()) == 23552 + 256 * 120
    assert case.frame == int(np.argmax(rec["voxels"])) and int(rec["voxels"][case.frame]) == 23552
    assert rec["lo"][case.frame].tolist() == [0, 0, 0] and rec["hi"][case.frame].tolist() == [S, S, S]
    others = np.delete(np.arange(257), case.frame)
    assert (rec["voxels"][others] == 120).all()
    assert ((rec["hi"][others].astype(np.int64) - rec["lo"][others]) == [5, 4, 6]).all()
    assert np.array_equal(cases.frame_and_blocks(64), cases.frame_and_blocks(128)[:64, :64, :64])


def test_restated_geometry():
    assert cases.box_word_items((0, 0, 0), (S, S, S)) == 64 * 64 * 17 == 69632
    assert cases.box_word_items((0, 0, 0), (32, 32, 32)) == 16 * 16 * 5
    assert cases.box_word_items((3, 2, 7), (4, 3, 8)) == 1 and cases.box_word_items((3, 2, 7), (4, 3, 9)) == 2     # one brick; two, which may lie in two words
    assert cases.posed_grid(257, S) == (63, 257)
    assert cases.posed_grid(100, S) == (163, 100)
    assert cases.posed_grid(5000, S) == (4, 4096)
    assert cases.posed_grid(1, S) == (272, 1) and cases.posed_grid(80, S) == (204, 80)
    assert cases.posed_grid(60, S)[0] == 272 and cases.posed_grid(61, S)[0] == 268       # the grid strides from 61 rows on
    assert cases.posed_grid(1, 32) == (5, 1) and cases.posed_grid(3276, 32)[0] == 5 and cases.posed_grid(3277, 32)[0] == 4
    gx, _ = cases.posed_grid(257, S)
    assert gx * cases.GROUP < cases.box_word_items((0, 0, 0), (S, S, S))
    # the walk takes every item once, whatever the grid, and a whole-volume box has no item beyond its rows' words
    for items, groups in ((69632, 63), (69632, 4), (69632, 272), (1280, 5), (1000, 3), (7, 2)):
        w = cases.walk(items, groups)
        assert np.array_equal(np.sort(w[:, 2]), np.arange(items))
        assert (w[:, 2] == w[:, 0] + w[:, 1] * groups * cases.GROUP).all()
    cx, cy, kz, valid = cases.item_words((0, 0, 0), (S, S, S), S)
    assert (kz[valid] < 16).all() and int(valid.sum()) == 64 * 64 * 16 and not valid[16::17].any()
    # an odd box: the decoded words are exactly the words its voxels lie in
    lo, hi = (5, 2, 13), (40, 9, 100)
    cx, cy, kz, valid = cases.item_words(lo, hi, S)
    x, y, z = np.meshgrid(np.arange(lo[0], hi[0]), np.arange(lo[1], hi[1]), np.arange(lo[2], hi[2]), indexing="ij")
    want = set(zip((x >> 1).ravel().tolist(), (y >> 1).ravel().tolist(), (z >> 3).ravel().tolist()))
    got = list(zip(cx[valid].tolist(), cy[valid].tolist(), kz[valid].tolist()))
    assert len(got) == len(set(got)) and set(got) == want


def test_the_poses_are_what_the_gpu_tests_rely_on():
    case = cases.large_case()
    points = cases.large_points()
    frame = points[case.frame]
    assert len(frame) == 18485 and case.boxes[case.frame].tolist() == WHOLE
    assert case.keep[case.frame] == 1 and 0.7 < case.keep.mean() < 0.9 and not case.keep.all()
    # four more whole-volume boxes, in different octants of the destination
    assert len(case.whole) == 4 and case.frame not in case.whole
    octants = set()
    for i in case.whole:
        assert case.boxes[i].tolist() == WHOLE and case.keep[i] == 1 and len(points[i]) > 60
        octants.add(tuple((points[i].mean(0) >= S / 2).tolist()))
    assert len(octants) == 4
    # the odd rows
    odd = case.odd
    assert stamp_model.clip_box(S, case.boxes[odd["empty"]][:3], case.boxes[odd["empty"]][3:]) is None
    assert case.boxes[odd["inverted"]][0] > case.boxes[odd["inverted"]][3]
    assert (case.boxes[odd["clipped"]][3:] == 0xFFFFFFFF).all() and len(points[odd["clipped"]]) > 60
    assert all(case.keep[i] == 1 for i in odd.values())
    for name in ("empty", "inverted", "outside"):
        assert len(points[odd[name]]) == 0, name
    shifted = (case.maps[odd["outside"]][0], [v - (300 << 17) for v in case.maps[odd["outside"]][1]])
    assert len(cases.posed_points(case.ids, odd["outside"], shifted, case.boxes[odd["outside"]], S)) > 60
    # generous boxes: the other blocks lose nothing to theirs
    for i in (20, 100, 255, 256):
        assert case.keep[i] and i not in case.whole and i not in odd.values()
        assert len(cases.posed_points(case.ids, i, case.maps[i], None, S)) == len(points[i]) > 60
    # the blocks meet the frame and each other, the frame reaches the faces
    pairs = cases.large_pairs()
    with_frame = cases.pair_records_of(points, [p for p in pairs.tolist() if p[0] == case.frame], S)
    between = cases.pair_records_of(points, [p for p in pairs.tolist() if case.frame not in p][::10], S)
    assert sum(r[1] > 0 for r in with_frame) > 20 and sum(r[4] > 0 for r in with_frame) > 20
    assert sum(r[1] > 0 for r in between) > 5 and sum(r[4] > 0 for r in between) > 5
    walls = contact_model.record_at(frame, contact_model.walled(np.zeros((S, S, S), np.uint8)))
    assert walls[4] > 100 and all(v != 0 for v in walls[6])


def test_a_lane_carries_sums_from_one_iteration_to_the_next():
    """the frame under its map in posed_grid(257), (100) and (5000 pairs): some lane adds posed voxels in at least two
    iterations of its stride loop; summed the way the kernels walk the items, nothing is lost or counted twice"""
    case = cases.large_case()
    frame = cases.large_points()[case.frame]
    counts = cases.item_counts(frame, WHOLE, S)
    assert int(counts.sum()) == len(frame)
    for rows, at_least in ((257, 1), (100, 1), (5000, 1024)):
        gx, gy = cases.posed_grid(rows, S)
        assert gx * cases.GROUP < len(counts)
        carrying, busy = cases.carrying_lanes(frame, WHOLE, gx, S)
        print("rows %d: grid %d x %d, %d of %d lanes with posed voxels carry them over iterations (%.0f %%)" % (rows, gx, gy, carrying, busy, 100.0 * carrying / busy))
        assert carrying >= at_least
        w = cases.walk(len(counts), gx)
        assert int(w[:, 1].max()) + 1 == -(-len(counts) // (gx * cases.GROUP))
        assert int(counts[w[:, 2]].sum()) == len(frame)
    # a workgroup of the frame's row that gathers nothing, next to ones that do: contact_flush's early exit is taken
    gx, _ = cases.posed_grid(257, S)
    w = cases.walk(len(counts), gx)
    per_group = np.bincount(w[:, 0] // cases.GROUP, weights=counts[w[:, 2]], minlength=gx)
    blocks_rows = cases.large_points()[20]
    small = cases.item_counts(blocks_rows, case.boxes[20], S)
    ws = cases.walk(len(small), gx)
    small_groups = np.bincount(ws[:, 0] // cases.GROUP, weights=small[ws[:, 2]], minlength=gx)
    assert (per_group > 0).all() and (small_groups > 0).any() and (small_groups == 0).any()


def test_the_broad_phase_has_runs_on_both_sides_of_its_workgroup_boundary():
    case = cases.large_case()
    pairs = cases.large_pairs()
    a = pairs[:, 0].astype(np.int64)
    assert len(pairs) > 2000
    assert (a == 255).sum() >= 3 and (a == 256).sum() >= 3 and (a < 255).any()
    first, capacity = cases.boundary_window(pairs)
    assert capacity >= 3 and first + capacity < len(pairs)
    assert a[first] < 256 and a[first - 1] == a[first]                       # starts inside the run of a piece of the first workgroup
    last = first + capacity - 1
    assert a[last] == 256 and a[last + 1] == 256 and a[last - 1] == 256      # ends inside the run of piece 256, the second workgroup's
    assert case.keep[255] == 1 and case.keep[256] == 1
    # the frame's run has every kept piece with a box
    live = sum(1 for i in range(257) if case.keep[i] and pair_contact_model.clipped(case.boxes[i], S))
    assert (a == case.frame).sum() == live - 1


def test_models_agree_at_this_size():
    case = cases.large_case()
    points = cases.large_points()
    only = np.zeros(257, np.uint8)
    only[case.frame] = 1
    dense = contact_model.posed(case.ids, case.frame, case.maps[case.frame], case.boxes[case.frame], S)
    placed = rigid_model.place_affine(case.ids, case.maps, case.boxes, np.zeros((S, S, S), np.uint8), rigid_model.OR, only)
    assert np.array_equal(placed, dense)
    assert np.array_equal(np.argwhere(dense), points[case.frame])
    some = [case.frame, case.whole[0], case.odd["clipped"], case.odd["outside"], case.odd["empty"], 30, 256]
    some += [int(np.flatnonzero(case.keep == 0)[0])]
    keep = np.zeros(257, np.uint8)
    keep[some] = case.keep[some]
    sets = contact_model.posed_sets(case.ids, case.maps, case.boxes, S, keep)
    for i in some:
        if case.keep[i]:
            assert np.array_equal(np.argwhere(sets[i]), points[i]), i
        else:
            assert sets[i] is None and points[i] is None
    name, world = contact_model.worlds(S, 3)[0]
    star = contact_model.walled(world)
    fast = cases.contacts_of(points, world)
    assert [fast[i] for i in some] == [contact_model.record(sets[i], star) for i in some]
    pairs = [(case.frame, 30), (30, case.frame), (case.whole[0], case.frame), (30, some[-1]), (some[-1], 30), (30, 257), (300, 30), (256, 256)]
    assert cases.pair_records_of(points, pairs, S) == pair_contact_model.records_of(sets, pairs, S)
    # the moments on a crop the brute-force loop can take
    crop = np.ascontiguousarray(case.ids[:32, :32, :32])
    C = int(crop[crop != cases.NONE].max()) + 1
    assert C > 4
    assert [(n, list(s1), list(s2)) for n, s1, s2 in rigid_model.moments_fast(crop, C)] == [(n, s1, s2) for n, s1, s2 in rigid_model.moments(crop, C)]


def test_scaled_case_strides_too():
    case = cases.scaled_case()
    C = len(case.rec)
    assert C == 129 and case.ids.shape == (64, 64, 64) and case.Sd == S
    gx, gy = cases.posed_grid(C, S)
    assert C >= 61 and gx * cases.GROUP < cases.box_word_items((0, 0, 0), (S, S, S))
    frame = cases.posed_points(case.ids, case.frame, case.maps[case.frame], case.boxes[case.frame], S)
    assert case.boxes[case.frame].tolist() == WHOLE and case.keep[case.frame] == 1 and len(frame) > 10000
    carrying, busy = cases.carrying_lanes(frame, WHOLE, gx, S)
    print("scaled: grid %d x %d, %d of %d busy lanes carry" % (gx, gy, carrying, busy))
    assert carrying >= 1
    shown = 0
    for i in range(1, C, 9):
        p = cases.posed_points(case.ids, i, case.maps[i], case.boxes[i], S)
        assert len(p) == len(cases.posed_points(case.ids, i, case.maps[i], None, S))      # place_box's boxes are generous
        shown += len(p) > 0
    assert shown > 8
