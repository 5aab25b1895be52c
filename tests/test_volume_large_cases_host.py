"""The cases of tests/test_gpu_volume_large.py without a GPU (tests/large_volume_cases.py): the launch geometry restated there
puts the scan of the labelling into its second step, the one-box kernels into a second iteration of their grid stride and
the many-box kernels into a second iteration over gridDim.y; the later steps meet something that matters (roots, bits the
operation changes, solid voxels to count); and the expected labelling of 256^3, made of parts, is components_model.label's
where that can be run.  If the restated geometry stops matching the code, update the restatement; the conditions stay."""
import numpy as np

import components_model
import large_volume_cases as cases
import stamp_model

NONE = cases.NONE


# ---- the restated geometry --------------------------------------------------------------------------------------------

def test_restated_geometry():
    assert [cases.groups_of(d) for d in (4, 6, 7, 8)] == [1, 32, 256, 2048]
    assert [cases.scan_steps(n) for n in (1, 32, 256, 1024, 1025, 2048)] == [1, 1, 1, 1, 2, 2]
    counts = np.arange(2500) % 7
    prefix, total = cases.scan_slots(counts)
    assert np.array_equal(prefix, np.cumsum(counts) - counts) and total == int(counts.sum())
    broken, _ = cases.scan_slots(counts, carry=False)
    assert np.array_equal(broken[:1024], prefix[:1024]) and (broken[1024:] < prefix[1024:]).all()
    whole = lambda S: ((0, 0, 0), (S, S, S))
    assert cases.box_word_items(*whole(256)) == 540672 and cases.box_launch_groups(*whole(256)) == 2112
    assert cases.box_word_items(*whole(512)) == 4259840 and cases.box_launch_groups(*whole(512)) == 16384
    assert cases.box_launch_groups((0, 0, 0), (1, 1, 1)) == 1
    # later_items and second_lanes are the stride loop's: walk's rows beyond the first iteration
    for items, groups in ((9216, 32), (1000, 1), (700, 3), (256, 1), (5, 1)):
        w = cases.walk(items, groups)
        assert np.array_equal(np.sort(w[w[:, 1] >= 1, 2]), cases.later_items(items, groups * cases.GROUP))
        assert int((w[:, 1] == 1).sum()) == cases.second_lanes(items, groups * cases.GROUP)
    assert [cases.split_for(6, n) for n in (1, 3, 128, 129, 4096, 4097, 5000)] == [32, 32, 32, 32, 1, 1, 1]
    assert [cases.split_for(d, 1) for d in (2, 4, 5, 6, 7, 8, 9)] == [1, 1, 4, 32, 256, 1024, 1024]
    # words_of: the later items of a whole-volume box at 64^3 under 8192 lanes are the rows from brick x = 28 on
    words = cases.words_of((0, 0, 0), (64, 64, 64), 64, cases.later_items(9216, 8192))
    rows = np.flatnonzero(words.any(axis=(1, 2)))
    assert rows.tolist() == [28, 29, 30, 31]
    assert int(words.sum()) == 1024 - sum(1 for it in range(8192, 9216) if it % 9 == 8)     # a row of 9 items has 8 words
    assert not words[28, :14].any() and words[28, 15:].all() and words[29:].all()
    a, b = np.zeros((64, 64, 64), np.uint8), np.zeros((64, 64, 64), np.uint8)
    b[55:, 3::7, ::3] = 1
    b[10, 10, 10] = 1
    by_hand = sum(1 for x, y, z in np.argwhere(b).tolist() if words[x >> 1, y >> 1, z >> 3])
    assert 0 < by_hand < int(b.sum()) and cases.differing_in(words, a, b) == by_hand


# ---- 1. the labelling ---------------------------------------------------------------------------------------------------

def test_the_construction_from_parts_is_the_models_labelling():
    """64^3 parts in 128^3, both connectivities: the assembled labelling is components_model.label of the assembled volume"""
    part = cases.part_scene(64)
    extras = cases.extras_for(part)
    vol = cases.assemble(part, extras)
    assert len(extras) == 2 * (4 * 5 + 2) + 2
    for connectivity in (6, 26):
        part_ids, part_rec = components_model.label(part, connectivity)
        ids, rec = cases.assembled_labelling(part, part_ids, extras, connectivity)
        want_ids, want_rec = components_model.label(vol, connectivity)
        assert 8 * len(part_rec) - len(rec) >= 4                       # the bars merged pieces
        assert np.array_equal(ids, want_ids), connectivity
        assert rec.tobytes() == want_rec.tobytes(), connectivity


def test_labelling_scene_takes_the_scan_into_its_second_step():
    case = cases.labelling_case()
    S = 256
    boundary = S ** 3 // 2                                                # key 2^23 = 1024 slots of 8192 keys
    assert case.vol.shape == (S, S, S) and cases.groups_of(8) == 2048 and cases.scan_steps(2048) == 2
    assert boundary == 1 << 23 == cases.SCAN_GROUP * cases.GROUP_KEYS
    K = components_model.keys(S)
    assert K[127, 255, 255] == boundary - 1 and K[128, 0, 0] == boundary
    for connectivity, pieces in ((6, 39960), (26, 16956)):
        ids, rec = case.ids[connectivity], case.rec[connectivity]
        assert len(rec) == pieces
        assert int(rec["voxels"].sum()) == int(case.vol.sum()) and np.array_equal(ids != NONE, case.vol != 0)
        slots = cases.root_slots(rec, S)
        assert (np.diff(slots) >= 0).all()                                  # ids ascend with the root key
        per_slot = np.bincount(slots, minlength=2048)
        below, above = int(per_slot[:1024].sum()), int(per_slot[1024:].sum())
        print("connectivity %d: %d roots below slot 1024, %d at or above; slot 1023 holds %d, slot 1024 %d; most in one slot %d"
              % (connectivity, below, above, per_slot[1023], per_slot[1024], per_slot.max()))
        assert below > 1000 and above > 1000 and below + above == pieces
        assert (per_slot[:1024] > 1).any() and (per_slot[1024:] > 1).any()
        assert per_slot[1023] >= 1 and per_slot[1024] >= 1
        # the carry is what numbers the upper half: without it every id there is too small by `below`
        prefix, total = cases.scan_slots(per_slot)
        assert total == pieces and prefix[1024] == below
        assert cases.scan_slots(per_slot, carry=False)[0][1024] == 0
        # a piece with voxels on both sides of the boundary and its root below; a piece wholly above
        keys_of = K[case.vol != 0]
        piece_of = ids[case.vol != 0].astype(np.int64)
        low, high = np.full(pieces, boundary * 2), np.zeros(pieces, np.int64)
        np.minimum.at(low, piece_of, keys_of)
        np.maximum.at(high, piece_of, keys_of)
        straddling = int(((low < boundary) & (high >= boundary)).sum())
        assert straddling >= 1 and int((low >= boundary).sum()) == above
        # the bars joined pieces across the boundary, the specks are pieces of one voxel in slots 1023 and 1024
        bar_pieces = ids[tuple(case.extras.T)].astype(np.int64)
        assert (bar_pieces != NONE).all()
        specks = [i for i in np.unique(bar_pieces) if rec["voxels"][i] == 1 and slots[i] in (1023, 1024)]
        assert sorted(int(slots[i]) for i in specks) == [1023, 1024]


def test_serpentine_is_one_piece_through_every_workgroup():
    vol, rec = cases.serpentine_case(128)
    assert int(vol.sum()) == int(rec["voxels"][0]) == 528383
    xyz = np.argwhere(vol)
    assert xyz.min(0).tolist() == rec["lo"][0].tolist() == [0, 0, 0] and (xyz.max(0) + 1).tolist() == rec["hi"][0].tolist() == [127, 127, 128]
    assert cases.groups_of(7) == 256
    assert len(np.unique(components_model.keys(128)[vol != 0] // cases.GROUP_KEYS)) == 256
    small, small_rec = cases.serpentine_case(32)                            # the closed form, held to the model where that is quick
    ids, model_rec = components_model.label(small, 6)
    assert model_rec.tobytes() == small_rec.tobytes()


# ---- 2. one box at 512^3 ------------------------------------------------------------------------------------------------

def test_one_box_cases_stride_and_their_second_words_matter():
    """every 512^3 launch: the items against the cap, the lanes that take a second word, and the voxels that the operation
    changes inside those second words; the control stays below the cap"""
    cap = cases.BOX_GROUPS * cases.GROUP
    assert cap == 16384 * 256
    seen = {}
    for name, lo, hi, op, second, before, after in cases.one_box_cases():
        items = cases.box_word_items(lo, hi)
        groups = cases.box_launch_groups(lo, hi)
        assert cases.second_lanes(items, groups * cases.GROUP) == second, name
        if name.startswith("copy control"):
            assert items == 252 * 256 * 65 <= cap and groups == 16380 and second == 0
            continue
        assert items > cap and groups == cases.BOX_GROUPS and second > 0, name
        words = cases.words_of(lo, hi, cases.BIG, cases.later_items(items, cap))
        a, b = before(), after()
        changed = cases.differing_in(words, a, b)
        print("%s op %d: %d items, %d lanes take a second word, %d voxels change there, %d in all" % (name, op, items, second, changed, int((a != b).sum())))
        seen[name, op] = changed
        assert changed > 1000, name
        # the first workgroup's worth of second words alone: what a stride one workgroup too long would leave out
        first_group = cases.words_of(lo, hi, cases.BIG, np.arange(cap, cap + cases.GROUP))
        assert cases.differing_in(first_group, a, b) > 0, name
    assert len(seen) == 7


def test_the_slice_models_are_stamp_models():
    """copied and shifted against stamp_model.stamp at 64^3, clipped boxes and all three ops"""
    rng = np.random.default_rng(9)
    src, dst = (rng.random((64, 64, 64)) < 0.3).astype(np.uint8), (rng.random((64, 64, 64)) < 0.5).astype(np.uint8)
    for op in (cases.REPLACE, cases.OR, cases.ANDNOT):
        for d, lo, hi in (((-3, 5, -7), (1, 0, 5), (64, 61, 64)), ((0, 0, 0), (0, 0, 0), (64, 64, 64)), ((70, 0, 0), (2, 2, 2), (9, 9, 9)), ((1, -1, -1), (1, 1, 1), (63, 63, 63))):
            want = stamp_model.stamp(dst, src, stamp_model.IDENTITY[0], [v << 17 for v in d], lo, hi, op)
            assert np.array_equal(cases.shifted(dst, src, d, lo, hi, op), want), (op, d)
        for src_lo, size, dst_lo in (((2, 0, 0), (62, 62, 62), (1, 1, 1)), ((0, 0, 0), (64, 64, 64), (0, 0, 0)), ((5, 6, 7), (80, 20, 30), (-2, 50, 3))):
            lo, hi, off = cases.copy_box(src_lo, size, dst_lo, 64, 64)
            want = stamp_model.stamp(dst, src, stamp_model.IDENTITY[0], [v << 17 for v in off], lo, hi, op)
            assert np.array_equal(cases.copied(dst, src, src_lo, size, dst_lo, op), want), (op, src_lo)
    m, t = stamp_model.signed_permutation(*cases.TURN, 64)
    assert np.array_equal(stamp_model.permuted(src, *cases.TURN), stamp_model.stamp(np.zeros_like(src), src, m, t))
    m, t, lo, hi, d = cases.placed_case()
    assert d == [-3, 5, -7] and lo == [1, 0, 5] and hi == [512, 509, 512]


# ---- 3. many boxes ------------------------------------------------------------------------------------------------------

def test_many_box_launches_stride():
    """split_for (vrc_volume.hip) caps gridDim.y at `useful` = the groups that cover the volume's WORDS once, but a box
    has up to one item more per brick row than its row has words (wpr, vrc_box_words.h:84): a whole-volume box strides
    whenever split_for reaches `useful`, from 32^3 on, and any box of more than 256 items strides in a list of 4096 or more.
    The suite had such launches already -- fillBoxes of one whole-volume box at 64^3 in test_gpu_volume_components.py, a
    sphere over everything at 32^3 and 256^3 in test_gpu_volume_brushes.py -- and here is that they do stride"""
    for depth in (5, 6, 8):
        assert cases.split_for(depth, 1) * cases.GROUP < cases.whole_box_items(depth), depth
    assert cases.split_for(4, 1) * cases.GROUP >= cases.whole_box_items(4)
    case = cases.many_box_case()
    S = 1 << cases.MANY_DEPTH
    base = cases.dense_of(case.base_edits, S)
    # few: the whole-volume box and the sphere over everything take 1024 second words each, and filling changes voxels there
    lanes = cases.split_for(cases.MANY_DEPTH, 3) * cases.GROUP
    assert lanes == 8192
    for lo, hi in (((0, 0, 0), (S, S, S)), cases.sphere_box(S, case.few_spheres[0])):
        items = cases.box_word_items(lo, hi)
        assert items == 9216 and cases.second_lanes(items, lanes) == 1024
        words = cases.words_of(lo, hi, S, cases.later_items(items, lanes))
        assert cases.differing_in(words, base, np.ones_like(base)) > 20000
    assert cases.second_lanes(cases.box_word_items(case.few_boxes[1, :3], case.few_boxes[1, 3:]), lanes) > 0
    filled = base.copy()
    cases.fill_spheres(filled, case.few_spheres[:1], 1)
    assert filled.all()
    # many: 256 lanes a box
    assert len(case.many_boxes) == 4101 and cases.split_for(cases.MANY_DEPTH, 4100) == 1 and cases.split_for(cases.MANY_DEPTH, 4101) == 1
    striding = changed = 0
    full = np.ones_like(base)
    for b in case.many_boxes[:4100:41].astype(np.int64):
        lo, hi = stamp_model.clip_box(S, b[:3], b[3:])
        items = cases.box_word_items(lo, hi)
        if items <= cases.GROUP:
            continue
        striding += 1
        words = cases.words_of(lo, hi, S, cases.later_items(items, cases.GROUP))
        cleared = full.copy()
        cleared[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 0
        changed += cases.differing_in(words, full, cleared) > 0
    print("many boxes: %d of 100 sampled stride, %d of them clear voxels in later words" % (striding, changed))
    assert striding >= 20 and changed == striding
    items = [cases.box_word_items(*box) for box in (cases.sphere_box(S, s) for s in case.many_spheres) if box is not None]
    assert sum(i > cases.GROUP for i in items) >= 500 and cases.split_for(cases.MANY_DEPTH, len(case.many_spheres)) == 1
    # the counts: the whole-volume box last in the long list takes 36 words a lane, solid ones among the later
    assert cases.whole_box_items(cases.MANY_DEPTH) == 36 * cases.GROUP
