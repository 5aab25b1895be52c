"""tests/columns_cases.py held to its regime without a GPU: the sparse model against columns_model on the dense form of the
catalogue, the word-by-word emulation of k_columns_profile / k_columns_select against the sparse model at every depth of
tests/test_gpu_volume_columns_planes.py, the planes the expected records reach, the placement over bundles and workgroups, and
for every wrong kernel of columns_cases.WRONG how much of the new cases it changes -- and how much of the scenes that
tests/test_gpu_volume_columns.py runs at 128^3, 256^3 and 1024^3.

What the old scenes miss (OLD below: zero records and zero voxels at all three sizes): a `runs` of 9 planes (1); first and last
read out with the planes 8 and 9 exchanged (3: both are 0 or S - 1 there, all planes equal); SIGNED_PLANES 11 (9): eleven planes
hold P - lo and P - hi modulo 2048, and of all the values -1025 .. 1023 only -1025 lands on the wrong side of the sign plane, so
the one band that shows it is (0, S + 1) at 1024^3 at the voxels with P = 0 -- the new select runs that band.
What they do notice, other than was supposed when the cases were asked for: add_bit's carry stopping after plane 5 (4: one
column in seventy of the random field at 128^3 holds 64 or more, and the full columns count past it); prev reset at every word
on the notched volumes (7: a full column then has a run per word, and the old test asks for runs == 1); from_hi initialised from
lo (11), which selects nothing at all, at every size.  The new cases notice every switch."""
import numpy as np
import pytest

import columns_cases as cc
import columns_model as model

DEPTHS = (7, 8, 9, 10)
KINDS = (model.SOLID, model.EMPTY, model.BOTH)


def kind_bands(S, every):
    """[(lo, hi, of)]: every `every`-th band of cc.bands with the kinds in turn, EMPTY and BOTH only with lo >= 1"""
    out = []
    for i, (lo, hi) in enumerate(cc.bands(S)[::every]):
        of = KINDS[i % 3]
        out.append((lo, hi, of if lo >= 1 else model.SOLID))
    return out


# ---- 1. the sparse model is the dense model --------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [6, 7])
def test_sparse_model_is_the_dense_model(depth):
    S = 1 << depth
    for axis in range(3):
        sc = cc.scene(depth, axis)
        vol = sc.dense()
        assert int(vol.sum()) == sc.solid() and np.array_equal(np.argwhere(vol), np.argwhere(cc.dense_of_words(sc.words())))
        for other in range(3):                                                 # the same voxels as columns of the other axes
            across = sc.seen_along(other)
            assert across.solid() == sc.solid() and (other != axis or sorted(across.columns) == sorted(sc.columns))
            for side in (0, 1):
                assert np.array_equal(across.profile(side), model.profile(vol, 2 * other + side)), (axis, other, side)
        (a, b), = [k for k in sc.placed if len(sc.placed[k]) == cc.N_COLUMNS[axis]][:1]
        for side in (0, 1):
            direction = 2 * axis + side
            assert np.array_equal(sc.profile(side), model.profile(vol, direction))
            for rect in cc.rects_around(axis, S, a, b):
                assert np.array_equal(sc.profile(side, rect), model.profile(vol, direction, rect)), rect
            for of in KINDS:
                for lo, hi in cc.bands(S)[::1 if depth == 6 else 5]:
                    if of != model.SOLID and lo < 1:
                        continue
                    want = model.selection(vol, direction, lo, hi, of)
                    assert np.array_equal(sc.selection_scene(side, lo, hi, of).dense(), want), (axis, side, lo, hi, of)
                    boxes, sizes = sc.selection_boxes(side, lo, hi, of)
                    assert int(sizes.sum()) == int(want.sum())
                    assert all(want[x0:x1, y0:y1, z0:z1].all() for x0, y0, z0, x1, y1, z1 in boxes.tolist())


def test_selected_spans_by_hand():
    runs = ((1, 2), (3, 4))                                                     # test_columns_host.py: column [0, 1, 0, 1]
    assert cc.selected_spans(runs, 4, 1, 0, 1, model.SOLID) == [(1, 2)] and cc.selected_spans(runs, 4, 0, 0, 1, model.SOLID) == [(3, 4)]
    assert cc.selected_spans(runs, 4, 1, 0, 1, model.EMPTY) == [(0, 1)] and cc.selected_spans(runs, 4, 1, 1, 5, model.EMPTY) == [(2, 3)]
    assert cc.selected_spans(runs, 4, 0, 1, 2, model.BOTH) == [(1, 3)] and cc.selected_spans(runs, 4, 1, 1, 1, model.BOTH) == []
    assert cc.record_tuple(runs, 4, 1) == (1, 3, 2, 2) and cc.record_tuple(runs, 4, 0) == (3, 1, 2, 2) and cc.record_tuple((), 4, 1) == cc.EMPTY_RECORD
    assert cc.normal([(5, 6), (1, 2), (2, 3)]) == ((1, 3), (5, 6))


# ---- 2. the emulation is the kernels' arithmetic ------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [4, 8, 16, 32])
def test_emulation_is_the_dense_model_on_random_fields(S):
    """every bundle of a small random volume, 4^3 with its half words included: the layout, level, walk_of and column_of"""
    rng = np.random.default_rng(S)
    vol = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    words = cc.Words.of_dense(vol)
    for axis in range(3):
        a, b = cc.all_bundles(axis, S)
        c = np.arange(cc.N_COLUMNS[axis])
        _, u, v = cc.column_of(axis, c[None, :], a[:, None], b[:, None])
        inside = (u < S) & (v < S)                                              # 4^3: the levels 4 .. 7 of a half
        for side in (0, 1):
            direction = 2 * axis + side
            got = cc.emulate_profile(words, axis, side, a, b)
            want = model.profile(vol, direction)
            want = np.stack([want[f].astype(np.int64) for f in ("first", "last", "count", "runs")], -1)
            assert np.array_equal(got[inside], want[u[inside], v[inside]]), (S, direction)
            assert (got[~inside] == np.array(cc.EMPTY_RECORD)).all()
            for lo, hi, of in [(0, 1, 1), (1, S // 2, 3), (2, S + 1, 2), (S // 2, 0xFFFFFFFF, 3), (3, 3, 3)]:
                K, index = cc.emulate_select(words, axis, side, lo, hi, of, a, b)
                sel = cc.Words.of_dense(model.selection(vol, direction, lo, hi, of))
                if S == 4:                                                      # a bundle has a half of the word
                    _, _, shift, step, mask, steps = cc.walk_of(axis, 0, a, b)
                    at = (shift[:, None] + np.arange(steps)[None, :] * step).astype(np.uint32)
                    assert np.array_equal(K, (sel[index] >> at) & np.uint32(mask)), (S, direction, lo, hi, of)
                else:
                    assert np.array_equal(K, sel[index]), (S, direction, lo, hi, of)


@pytest.mark.parametrize("depth", DEPTHS)
def test_emulation_is_the_sparse_model(depth):
    S = 1 << depth
    for axis in range(3):
        sc = cc.scene(depth, axis)
        for side in (0, 1):
            got, stray = cc.emulated_records(sc, side)
            assert np.array_equal(got, sc.records(side)) and stray == 0, (depth, axis, side)
            for lo, hi, of in kind_bands(S, 1 + 2 * (depth - 7) ** 2):
                assert cc.select_errors(sc, side, lo, hi, of) == 0, (depth, axis, side, lo, hi, of)


# ---- 3. the planes the cases reach ----------------------------------------------------------------------------------------------

def test_every_plane_holds_a_one_and_a_zero_at_depth_10():
    for axis in range(3):
        sc = cc.scene(10, axis)
        for side in (0, 1):
            rec = sc.records(side)
            rec = rec[rec[:, 2] > 0]
            for field, planes in ((0, cc.COORD_PLANES), (1, cc.COORD_PLANES), (2, cc.COUNT_PLANES), (3, cc.COORD_PLANES)):
                v = rec[:, field]
                assert v.max() < 1 << planes
                for p in range(planes):
                    one = (v >> p) & 1 == 1
                    assert one.any(), (axis, side, field, p)
                    if p + 1 < planes:
                        assert (~one & (v >> (p + 1) != 0)).any(), (axis, side, field, p)       # a zero under a one
                    if p:
                        assert (~one & (v & ((1 << p) - 1) != 0)).any(), (axis, side, field, p)   # a zero above a one


@pytest.mark.parametrize("depth", DEPTHS)
def test_the_catalogue_holds_what_it_must(depth):
    S = 1 << depth
    programs = dict((runs, name) for name, runs in cc.catalogue(S))
    assert len(programs) == len(cc.catalogue(S))                               # pairwise different
    assert all(0 <= z0 < z1 <= S for runs in programs for z0, z1 in runs)
    assert all(a[1] < b[0] for runs in programs for a, b in zip(runs, runs[1:]))               # disjoint and not adjacent
    comb = lambda r, start: tuple((start + 2 * i, start + 2 * i + 1) for i in range(r))
    for p in cc.powers(S):
        assert ((p - 1, p + 1),) in programs                                   # the pair (2^b - 1, 2^b): adjacent, one run of two
        assert ((p, p + 1), (S - 1, S)) in programs or p == S - 1              # the pair (2^b, S - 1)
        for r in (p - 1, p, p + 1):
            for start in (0, 1):
                assert (comb(r, start) in programs) == (r >= 1 and start + 2 * r - 1 <= S), (r, start)
            for c in (r, ) if r >= 1 else ():
                assert {((0, c),), ((S - c, S),), (((S - c) // 2, (S - c) // 2 + c),)} <= set(programs)
    assert comb(S // 2, 0) in programs and comb(S // 2, 1) in programs         # the top plane of runs
    assert ((0, S),) in programs                                               # the top plane of count
    twos = [runs for runs in programs if len(runs) > 2 and all(z1 - z0 == 2 for z0, z1 in runs)]
    assert len(twos) == 1 and len(twos[0]) == S // 4 + 1
    e, o = 8 * (7 * S // 64), 7 * S // 8 + 1
    assert e % 8 == 0 and e >= 3 * S // 4 and o & 1 and o >= 3 * S // 4        # a word seam along z; level 1 of a word along x, y
    for at in (e, o + 1):
        assert {((at - 3, at),), ((at, at + 3),), ((at - 2, at + 2),)} <= set(programs)


# ---- 4. the placement --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [6] + list(DEPTHS))
def test_placement(depth):
    S = 1 << depth
    for axis in range(3):
        sc = cc.scene(depth, axis)
        N = cc.N_COLUMNS[axis]
        na, nb = cc.face_bundles(axis, S)
        assert (na, nb) == ((S // 2, S // 2) if axis == 2 else (S // 2, S // 8))
        assert sorted(runs for _, _, runs in sc.columns) == sorted(runs for _, runs in cc.catalogue(S))      # every program, once
        for (a, b), held in sc.placed.items():
            assert 0 <= a < na and 0 <= b < nb
            for c, i in held.items():
                assert cc.column_of(axis, c, a, b)[1:] == sc.columns[i][:2] and cc.bundle_of(axis, *sc.columns[i][:2]) == (a, b, c)
        whole = [k for k, held in sc.placed.items() if len(held) == N]
        assert whole and all(len({sc.columns[i][2] for i in sc.placed[k].values()}) == N for k in whole)
        dealt, full = cc.bundle_lanes(axis, S, len(sc.columns))
        alone = [divmod(lane, nb) for lane in dealt[full:]]                    # one column each, at every position in turn
        assert [list(sc.placed[k]) for k in alone] == [[c] for c in range(N)] and len(sc.placed) == len(dealt)
        assert (na - 1, nb - 1) in whole                                       # the last bundle of the face, all columns programmed
        lanes = sorted(cc.lane_of(axis, S, a, b) for a, b in sc.placed)
        assert lanes[-1] == na * nb - 1 and min(np.diff(lanes)) >= 2           # empty bundles between any two
        groups = {lane // cc.WALK_GROUP for lane in lanes}
        assert len(groups) >= 2 and cc.groups_of(axis, (0, 0, S, S)) - 1 in groups
        assert len({b for _, b in sc.placed}) > 1 and len({a for a, _ in sc.placed}) > 1
        for a, b in sc.placed:                                                 # the small rects: the bundle is cut on every side
            r = cc.rects_around(axis, S, a, b)
            u0, v0, u1, v1 = cc.bundle_rect(axis, S, a, b)
            assert all(0 <= x[0] < x[2] <= S and 0 <= x[1] < x[3] <= S for x in r)
            assert {(x[0] > u0, x[1] > v0, x[2] < u1, x[3] < v1) for x in r[1:]} == {(True, False, False, False), (False, True, False, False),
                                                                                      (False, False, True, False), (False, False, False, True)}
            assert cc.bundles(axis, *r[0])[1] >= 2 and cc.bundles(axis, *r[0])[3] >= 2


def test_bands_open_and_close_in_different_words():
    for depth in DEPTHS:
        S = 1 << depth
        b = cc.bands(S)
        assert {lo for lo, _ in b} | {hi for _, hi in b} == set(cc.band_values(S)) and max(hi for _, hi in b) == S + 1
        assert all(0 <= lo and lo + 2 <= hi for lo, hi in b)                   # two solid voxels apart: never the same word along x, y
        assert any(hi - lo >= 16 for lo, hi in b) and (0, S + 1) in b          # (0, S + 1): the only band that needs the twelfth signed plane


# ---- 5. the wrong kernels ------------------------------------------------------------------------------------------------------

# the depth at which a wrong kernel can first change a result that the GPU file asks for (its select starts at depth 8)
FIRST_DEPTH = {1: 10, 2: 10, 3: 9, 4: 7, 5: 7, 6: 7, 7: 7, 8: 7, 9: 10, 10: 8, 11: 8, 12: 8, 13: 10}

# recorded results of the emulation on the committed cases, not tolerances.  NEW[w] = (records of the programmed columns that
# differ, both sides of the three axes; selected voxels that differ over pin_bands, both sides of the three axes) at
# FIRST_DEPTH[w].  OLD[w] = the same on the scenes of test_gpu_volume_columns.py at 128^3 (the random field: six whole-face
# profiles, its six selections), 256^3 and 1024^3 (the notched full volume: the bundles of its rect, its two selections).
NEW = {1: (12, 0), 2: (660, 0), 3: (594, 0), 4: (90, 0), 5: (414, 0), 6: (816, 0), 7: (370, 0), 8: (408, 0), 9: (0, 1230), 10: (0, 576),
       11: (0, 82398), 12: (0, 290), 13: (6, 0)}
OLD = {1: ((0, 0), (0, 0), (0, 0)), 2: ((0, 0), (0, 0), (1008, 0)), 3: ((0, 0), (0, 0), (0, 0)), 4: ((1412, 3371357), (1008, 704), (1008, 704)),
       5: ((58982, 0), (0, 0), (0, 0)), 6: ((98304, 0), (1008, 0), (1008, 0)), 7: ((95966, 0), (1008, 0), (1008, 0)),
       8: ((98304, 0), (64, 0), (64, 0)), 9: ((0, 0), (0, 0), (0, 0)), 10: ((0, 114688), (0, 544), (0, 544)),
       11: ((0, 3089813), (0, 704), (0, 704)), 12: ((0, 149471), (0, 64), (0, 64)), 13: ((0, 0), (0, 0), (944, 0))}


def pin_bands(S):
    b = cc.bands(S)
    return [(0, S + 1, model.SOLID), b[1] + (model.SOLID,), b[len(b) // 2] + (model.EMPTY,), b[-4] + (model.BOTH,), b[-1] + (model.SOLID,)]


def new_changes(wrong):
    depth = FIRST_DEPTH[wrong]
    records = voxels = 0
    for axis in range(3):
        sc = cc.scene(depth, axis)
        for side in (0, 1):
            if wrong in cc.PROFILE_SWITCHES:
                got, stray = cc.emulated_records(sc, side, wrong)
                records += int((got != sc.records(side)).any(-1).sum()) + stray
            if wrong in cc.SELECT_SWITCHES:
                voxels += sum(cc.select_errors(sc, side, lo, hi, of, wrong) for lo, hi, of in pin_bands(1 << max(depth, 8)) if depth >= 8)
    return records, voxels


@pytest.mark.parametrize("wrong", sorted(FIRST_DEPTH))
def test_wrong_kernel_changes_the_new_cases(wrong):
    got = new_changes(wrong)
    assert got == NEW[wrong] and sum(got) > 0, (cc.WRONG[wrong], got)


@pytest.mark.parametrize("wrong", sorted(FIRST_DEPTH))
def test_wrong_kernel_on_the_old_scenes(wrong):
    got = (cc.old_random_changes(wrong), cc.notch_changes(wrong, 8), cc.notch_changes(wrong, 10))
    assert got == OLD[wrong], (cc.WRONG[wrong], got)


def test_what_the_old_scenes_miss():
    missed = sorted(w for w, v in OLD.items() if v == ((0, 0), (0, 0), (0, 0)))
    assert missed == MISSED_BY_THE_OLD_SCENES
    assert set(cc.WRONG) == {0} | set(FIRST_DEPTH) == {0} | set(NEW) == {0} | set(OLD)


MISSED_BY_THE_OLD_SCENES = [1, 3, 9]
