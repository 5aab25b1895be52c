"""The cases of tests/test_gpu_volume_morph_large.py without a GPU (tests/morph_cases.py): the restated geometry of
k_morph_apply against a table written by hand, every dense case held to the regime it is meant for on the model's result --
never on a device result --, the word-wise model against morph_model.morph, and the sparse cases against their placement
conditions.  If the restated geometry stops matching csrc/vrc_morph.hip, update the restatement; the conditions stay.

Why the tuned source exists.  The solid fraction of the model's result for the cases of test_gpu_volume_morph.py
(named_elements() on model.source(64), outside = 0; whole result, then the least and the greatest of the eight 32^3 tiles), as
test_the_existing_cases_saturate prints them:
     1 offset              dilate 0.495 [0.24 .. 0.75]   erode 0.495 [0.24 .. 0.75]
     7 ball(1), cross      dilate 0.858 [0.71 .. 1.00]   erode 0.122 [0.00 .. 0.25]
     8 box 2x2x2           dilate 0.878 [0.74 .. 1.00]   erode 0.113 [0.00 .. 0.23]
     8 box 4x1x2           dilate 0.888 [0.77 .. 1.00]   erode 0.105 [0.00 .. 0.22]
     8 lines -3 .. 4       dilate 0.871 .. 0.877         erode 0.090 .. 0.109
     9 lines -4 .. 4       dilate 0.886 .. 0.897         erode 0.074 .. 0.094
    14 box 1x2x7           dilate 0.931 [0.83 .. 1.00]   erode 0.050 [0.00 .. 0.11]
    27 box 3x3x3           dilate 0.987 [0.97 .. 1.00]   erode 0.010 [0.00 .. 0.02]
    33 ball(2)             dilate 0.993 [0.98 .. 1.00]   erode 0.004 [0.00 .. 0.01]
    33 lines -16 .. 16     dilate 0.989 .. 0.992         erode 0.000 .. 0.003
    45 box 3x5x3           dilate 0.993 [0.98 .. 1.00]   erode 0.001 [0.00 .. 0.00]
   123, 257, 515 ball(3), ball(4), ball(5)   dilate 1.000 in every tile, erode 0.000 in every tile
From about thirty offsets upwards the expected result is one constant; a gather that loses columns, mask bits or pillars
gives the same constant.

The every-tile bound [0.03, 0.97] is asked of every case but those for which no source can meet it
(morph_cases.tile_bound_is_impossible).  In the four forms in which the ORed set reads present beyond the faces the result
at p is one constant wherever some sample of the element falls outside the volume, and where that holds for more than 97 %
of a tile's voxels the bound is out of reach whatever the source.  That is the case at 32^3 alone, for the eight elements
whose extent spans the volume (IMPOSSIBLE_AT_32, held below to the geometry), 32 of the 546 (element, size, form) cases;
their fractions are printed.  Every interior tile of every case is held to [0.35, 0.65]."""
import numpy as np
import pytest

import morph_cases as cases
import morph_model as model

DILATE, ERODE, SOLID, EMPTY = model.DILATE, model.ERODE, model.SOLID, model.EMPTY


def test_restated_geometry():
    # S: (tiles per axis, interior tiles of an axis, interior z blocks)
    by_hand = {4: (1, [], []), 8: (1, [], []), 16: (1, [], []), 32: (1, [], []), 64: (2, [], []), 128: (4, [1, 2], [1, 2]),
               256: (8, [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6]), 512: (16, list(range(1, 15)), list(range(1, 15))),
               1024: (32, list(range(1, 31)), list(range(1, 31)))}
    for S, row in by_hand.items():
        assert (cases.tiles(S), cases.interior_tiles(S), cases.interior_z_blocks(S)) == row, S
    assert cases.TILE == 16 and cases.SPAN == 32 and cases.tiles(1024) ** 3 == 32768
    # element: what -> (LX, LY, pitch), (k_lo, k_hi)
    e = np.array([(-16, -8, 9), (-9, 8, 16)])
    assert cases.staged(e, DILATE) == (39, 48, 24) and cases.byte_range(e, DILATE) == (0, 4)
    assert cases.staged(e, ERODE) == (39, 48, 24) and cases.byte_range(e, ERODE) == (3, 7)
    assert cases.staged(model.box(33, 33, 33), DILATE) == (64, 64, 40) and cases.byte_range(model.box(33, 33, 33), ERODE) == (0, 7)
    assert cases.staged([(0, 0, 0)], DILATE) == (32, 32, 24) and cases.byte_range([(0, 0, 0)], DILATE) == (2, 5)
    assert cases.staged([(0, 0, 0), (0, 17 - 16, 0), (0, -16, 0)], ERODE)[1:] == (49, 40)
    assert cases.columns(model.ball(2)) == 13 and cases.mask_bits(model.ball(2)) == 5 and cases.columns(model.line(2, -16, 16)) == 1
    assert cases.tile_of([(31, 32, 1023)]).tolist() == [[0, 1, 31]]
    k = np.zeros((64, 64, 64), np.uint8)
    k[32:, :32, 32:48] = 1
    assert cases.tile_fractions(k)[1, 0, 1] == 0.5 and cases.tile_fractions(k).sum() == 0.5 and len(cases.interior_fractions(k)) == 0


def test_every_required_element_is_there():
    e = cases.elements()
    assert sorted(e) == sorted(cases.NAMES)
    assert [len(e["ball%d" % r]) for r in range(2, 7)] == [33, 123, 257, 515, 925]
    assert (len(e["box3"]), len(e["box9"]), len(e["slab33"])) == (27, 729, 1089) and (e["slab33"][:, 1] == -5).all()
    for axis in range(3):
        line = e["line%d" % axis]
        assert len(line) == 33 and line[:, axis].min() == -16 and line[:, axis].max() == 16
    for n in (48, 200, 400):
        r = e["random%d" % n]
        assert len(r) == n and r.min() == -16 and r.max() == 16
    assert cases.columns(e["random400"]) > 256                                   # the column list beyond a workgroup's lanes
    assert max(cases.mask_bits(e[name]) for name in cases.NAMES) == 33 and cases.mask_bits(e["ball6"]) == 13
    one = e["one_sided"]
    assert one[:, 2].min() == 9 and one[:, 2].max() == 16 and one[:, 0].min() == -16 and one[:, 0].max() == -9
    assert cases.byte_range(one, ERODE) == (3, 7) and cases.byte_range(one, DILATE) == (0, 4)
    assert cases.byte_range(e["one_sided_reflected"], DILATE) == (3, 7) and cases.byte_range(e["one_sided_reflected"], ERODE) == (0, 4)
    assert cases.staged(e["wy16"], DILATE)[1:] == (48, 24) and cases.staged(e["wy17"], DILATE)[1:] == (49, 40)
    assert cases.staged(e["lx64"], ERODE)[0] == 64 and cases.staged(e["lx33"], DILATE)[0] == 33
    piece = cases.piece_shape()
    assert piece.shape == (16, 16, 16) and piece.sum() == len(e["piece"]) and np.abs(e["piece"]).max() <= 16
    # two forms of every element at 256^3, every form by some element, both sources by every element
    at_256 = [cases.forms_of(name, 256) for name in cases.NAMES]
    assert all(len(f) == 2 and cases.ored_is_sparse_solid(*f[0][:2]) != cases.ored_is_sparse_solid(*f[1][:2]) for f in at_256)
    assert {f for pair in at_256 for f in pair} == set(cases.COMBOS) and all(cases.forms_of(name, 128) == cases.COMBOS for name in cases.NAMES)
    assert len({cases.seed_of(name, S) for name in cases.NAMES for S in cases.SIZES}) == len(cases.NAMES) * len(cases.SIZES)


def test_the_word_wise_model_is_the_model():
    """morph_words against morph: every element in two forms at 64^3, and at 128^3 those whose z extent is one-sided or whole,
    the one of more than 256 columns and the one of pitch 40"""
    for S, names in ((64, cases.NAMES), (128, ["one_sided", "line2", "random48", "piece", "random400", "wy17"])):
        for name in names:
            e = cases.elements()[name]
            for what, of, outside in cases.forms_of(name, 256):
                vol = cases.tuned_source(name, S, cases.ored_is_sparse_solid(what, of))
                assert np.array_equal(model.morph_words(vol, what, e, of, outside), model.morph(vol, what, e, of, outside)), (S, name, what, of, outside)
    e = cases.elements()["piece"] + np.array(cases.PIECE_PIVOT, np.int32)
    vol = cases.tuned_source("piece", 64, True)
    assert np.array_equal(model.morph_words(vol, ERODE, e, EMPTY, 1, cases.PIECE_PIVOT), model.morph(vol, ERODE, cases.elements()["piece"], EMPTY, 1))
    assert model.morph_words(vol, DILATE, []).sum() == 0 and model.morph_words(vol, ERODE, []).sum() == 64 ** 3


IMPOSSIBLE_AT_32 = ["line0", "line1", "line2", "random48", "random200", "random400", "slab33", "lx64"]


def test_the_tile_bound_is_out_of_reach_at_32_only():
    """tile_bound_is_impossible by the geometry alone: the four forms with faces that read solid, at 32^3, of the elements that
    span the volume -- and nowhere else"""
    for S in cases.SIZES:
        for name in cases.NAMES:
            e = cases.elements()[name]
            for what, of, outside in cases.forms_of(name, S):
                want = S == 32 and name in IMPOSSIBLE_AT_32 and cases.faces_read_solid(what, outside)
                assert cases.tile_bound_is_impossible(e, what, outside, S) == want, (name, S, what, of, outside)
    forced = cases.forced_fractions(model.line(0, -16, 16), DILATE, 32)
    assert forced.shape == (1, 1, 1) and forced[0, 0, 0] == 1.0                  # x - ex leaves [0, 32) for some ex at every x
    assert cases.forced_fractions(model.ball(2), ERODE, 64).max() == 1.0 - (30 / 32) ** 3
    assert cases.forced_fractions(model.box(33, 33, 33), DILATE, 128)[1:3, 1:3, 1:3].max() == 0.0      # the interior tiles see no face
    assert sum(len(cases.forms_of(name, S)) for name in cases.NAMES for S in cases.SIZES) == 546


def deciding(vol, what, of, e, S, tried=None):
    """per offset of `tried` (all of e with None): whether removing it alone changes the model's result inside an interior tile.  With B the set being
    ORed (A for DILATE, its complement for ERODE), the result at p changes exactly when that offset's sample is the only
    one of B there.  Looked for in the first two interior tiles of every axis, which see no face."""
    t = cases.interior_tiles(S)
    lo, hi = cases.SPAN * t[0], cases.SPAN * (t[min(1, len(t) - 1)] + 1)
    a = (vol != 0) if of == SOLID else (vol == 0)
    b = a if what == DILATE else ~a
    sign = -1 if what == DILATE else 1

    def sample(o):
        return b[lo + sign * o[0]:hi + sign * o[0], lo + sign * o[1]:hi + sign * o[1], lo + sign * o[2]:hi + sign * o[2]]

    count = np.zeros((hi - lo,) * 3, np.uint16)
    for o in e.tolist():
        count += sample(o)
    alone = count == 1
    return [bool((sample(o) & alone).any()) for o in (e if tried is None else tried).tolist()]


def sample_of(name, e):
    """the offsets whose removal is tried: all of them, or 16 with the six extreme ones among them"""
    if name not in cases.SAMPLED:
        return e
    extreme = {int(i) for axis in range(3) for i in (e[:, axis].argmin(), e[:, axis].argmax())}
    rng = np.random.default_rng(len(e))
    while len(extreme) < 16:
        extreme.add(int(rng.integers(0, len(e))))
    return e[sorted(extreme)]


@pytest.mark.parametrize("S", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_dense_cases_are_unsaturated_and_every_offset_matters(name, S):
    e = cases.elements()[name]
    for what, of, outside in cases.forms_of(name, S):
        sparse = cases.ored_is_sparse_solid(what, of)
        vol = cases.tuned_source(name, S, sparse)
        d = cases.density_of(len(e))
        assert abs(vol.mean() - (d if sparse else 1.0 - d)) < 5.0 * np.sqrt(d / S ** 3)
        k = model.morph_words(vol, what, e, of, outside)
        every, inner = cases.tile_fractions(k), cases.interior_fractions(k)
        print(name, S, (what, of, outside), "tiles %.3f .. %.3f" % (every.min(), every.max()),
              "interior %.3f .. %.3f" % (inner.min(), inner.max()) if len(inner) else "no interior tile")
        if not cases.tile_bound_is_impossible(e, what, outside, S):
            assert every.min() >= 0.03 and every.max() <= 0.97, (name, S, what, of, outside, every.min(), every.max())
        assert len(inner) == len(cases.interior_tiles(S)) ** 3
        if len(inner):
            assert inner.min() >= 0.35 and inner.max() <= 0.65, (name, S, what, of, outside, inner.min(), inner.max())
            if outside == 0 or S == 256:                          # the interior sees no face: `outside` changes nothing there
                tried = sample_of(name, e)
                matters = deciding(vol, what, of, e, S, tried)
                assert all(matters), (name, S, what, of, tried[[i for i, m in enumerate(matters) if not m]].tolist())


def test_deciding_is_removal():
    """the shortcut of `deciding` against the model run with the offset taken out"""
    S, name = 128, "random48"
    e = cases.elements()[name]
    for what, of in ((DILATE, SOLID), (ERODE, SOLID), (DILATE, EMPTY)):
        vol = cases.tuned_source(name, S, cases.ored_is_sparse_solid(what, of))
        whole = model.morph_words(vol, what, e, of, 0)
        for i in (0, 17, 47):
            without = model.morph_words(vol, what, np.delete(e, i, axis=0), of, 0)
            assert deciding(vol, what, of, e, S)[i] == bool((whole != without)[32:96, 32:96, 32:96].any())
    solid = np.ones((S, S, S), np.uint8)                              # and an offset that decides nothing is seen as such
    assert not any(deciding(solid, DILATE, SOLID, e, S)) and not any(deciding(solid, ERODE, SOLID, e, S))


def test_interior_tiles_begin_at_128():
    for S in (128, 256):
        assert len(cases.interior_tiles(S)) >= 2 and cases.interior_z_blocks(S) == cases.interior_tiles(S)
        assert S // 2 != 32 and S // 8 != 8                         # brick rows and words per row are not the tile's constants
    assert (128 // 2, 128 // 8) != (256 // 2, 256 // 8)
    for S in (32, 64):
        assert cases.interior_tiles(S) == [] and cases.interior_z_blocks(S) == []


@pytest.mark.parametrize("S", [512, 1024])
def test_sparse_cases_meet_their_placement(S):
    p, T = cases.sparse_points(S), cases.tiles(S)
    assert 2000 <= len(p) <= 5000 and len(np.unique(p, axis=0)) == len(p) and p.min() == 0 and p.max() == S - 1
    chosen = cases.sparse_tiles(S)
    assert len(np.unique(chosen, axis=0)) == len(chosen) >= 64
    occupied = {tuple(t) for t in cases.tile_of(p).tolist()}
    assert {tuple(t) for t in chosen.tolist()} <= occupied
    for axis in range(3):
        assert {0, T - 1} <= {t[axis] for t in occupied}
        assert (p[:, axis] % 32 == 31).sum() >= 64 and (p[:, axis] % 32 == 0).sum() >= 64           # both sides of the seams
        assert (p[:, axis] == 0).any() and (p[:, axis] == S - 1).any()                              # the six faces
        mid = p[(p[:, axis] == 0) | (p[:, axis] == S - 1)]
        assert ((mid[:, (axis + 1) % 3] > 32) & (mid[:, (axis + 1) % 3] < S - 32)).any()            # and not at an edge only
    assert (p == S - 1).all(axis=1).any()
    local = [frozenset(map(tuple, cases.local_arrangement(i).tolist())) for i in range(len(chosen))]
    assert len(set(local)) == len(local)                          # a tile written to another tile's place shows
    for i, t in enumerate(chosen.tolist()):                       # and the volume holds exactly that arrangement there, or more
        here = p[(cases.tile_of(p) == t).all(axis=1)] - cases.SPAN * np.array(t)
        assert local[i] <= set(map(tuple, here.tolist()))
    depth = S.bit_length() - 1
    for name in cases.LARGE_ELEMENTS:
        e = cases.elements()[name]
        grown, holes = cases.dilated(p, e, S), cases.erosion_holes(p, e, S)
        for listed in (grown, holes):
            assert len(np.unique(listed, axis=0)) == len(listed) and listed.min() >= 0 and listed.max() < S
            assert np.array_equal(cases.in_list_order(listed, depth), listed)
        assert len(p) * len(e) // 2 < len(grown) < len(p) * len(e) and len(grown) < S ** 3 // 256          # sparse, and clipped at the faces
        assert {tuple(v) for v in p.tolist()} <= {tuple(v) for v in grown.tolist()}


def test_sparse_lists_are_the_dense_model():
    """dilated / erosion_holes against morph_model on a small volume with the same kind of content"""
    S = 64
    rng = np.random.default_rng(64)
    p = np.unique(np.concatenate([rng.integers(0, S, (60, 3)), [[0, 0, 0], [S - 1, S - 1, S - 1], [31, 32, 0]]]), axis=0)
    vol = np.zeros((S, S, S), np.uint8)
    vol[tuple(p.T)] = 1
    for name in cases.LARGE_ELEMENTS + ["one_sided"]:
        e = cases.elements()[name]
        assert np.array_equal(np.argwhere(model.morph(vol, DILATE, e)), np.unique(cases.dilated(p, e, S), axis=0))
        assert np.array_equal(np.argwhere(model.morph(1 - vol, ERODE, e, SOLID, 1) == 0), np.unique(cases.erosion_holes(p, e, S), axis=0))


def test_the_capped_list():
    e, rows = cases.capped_list()
    assert rows.shape == (1 << 20, 3) and rows.dtype == np.int32 and len(e) == 100
    key = lambda a: (a.astype(np.int64) + 16) @ np.array([33 * 33, 33, 1])       # noqa: E731
    counts = np.bincount(key(rows), minlength=33 ** 3)
    assert np.array_equal(np.flatnonzero(counts), np.sort(key(e))) and not np.array_equal(rows[:100], e)
    assert counts[counts > 0].min() >= 10485 and counts.max() <= 10486


def test_the_existing_cases_saturate():
    """the record of the module's docstring: printed, not asserted"""
    from test_gpu_volume_morph import named_elements
    vol = model.source(64)
    for e in named_elements():
        grown, shrunk = (cases.tile_fractions(model.morph(vol, what, e)) for what in (DILATE, ERODE))
        print("  %4d offsets, box %s: dilate %.3f [%.2f .. %.2f]   erode %.3f [%.2f .. %.2f]" % (
            len(e), (e.max(axis=0) - e.min(axis=0) + 1).tolist(), grown.mean(), grown.min(), grown.max(), shrunk.mean(), shrunk.min(), shrunk.max()))
