"""The cases of tests/test_gpu_volume_envelope.py without a GPU (tests/envelope_cases.py): the launch geometry restated there
puts the line loop of the min-plus kernels into its second step at 512^3 and the stacks into device memory at 256^3; the
scenes alone drive the restated first walk deep AND through pop cascades, under the distance field's rule and under the
fracture's strict one; the z pass of the fracture meets markers in all four chunks of a column; and the references agree
with the models of the small tests where those can be run.  These are conditions on the scenes, not measurements of the
kernels.  If the restated geometry stops matching the code, update the restatement; the conditions stay."""
import numpy as np
import pytest

import clearance_model
import components_model
import distance_model
import envelope_cases as cases
import fracture_model
import posed_cases
import stamp_model

NONE = cases.NONE


# ---- the restated geometry --------------------------------------------------------------------------------------------

def test_restated_geometry():
    # the line loop: one step up to 256^3, two at 512^3 on 256 compute units
    assert [cases.minplus_groups(d) for d in (2, 6, 7, 8, 9)] == [1, 64, 256, 1024, 2048]
    assert [cases.line_steps(d) for d in (6, 7, 8, 9, 10)] == [1, 1, 1, 2, 8]
    assert cases.line_steps(9, 304) == 2 and cases.line_steps(9, 512) == 1 and cases.line_steps(8, 120) == 2
    # the stacks: LDS up to 128^3 (64 lanes x 128 entries x 4 bytes = 32 KiB), device memory from 256^3
    assert cases.stacks_in_lds(7) and not cases.stacks_in_lds(8)
    assert cases.LANES * 4 << cases.LDS_STACK_MAX_DEPTH == 32768
    # k_distance_z strides at depths 7 and 8: 8192 workgroups wanted, 4096 launched; 4 and 8 words a column
    assert cases.distance_z_groups(7) == (8192, 4096) and cases.distance_z_groups(8) == (8192, 4096) and cases.distance_z_groups(6) == (1024, 1024)
    assert [cases.z_columns_per_step(S) for S in (4, 64, 128, 256, 512, 1024)] == [64, 4, 2, 8, 4, 2]
    assert [cases.words_per_column(S) for S in (4, 32, 128, 256)] == [1, 1, 4, 8]
    assert all(cases.z_columns_per_step(S) * cases.words_per_column(S) <= 64 for S in (4, 8, 16, 32, 64, 128, 256, 512, 1024))
    # k_fracture_z: a column is 2 chunks of a wave at 128^3 and 4 at 256^3
    assert cases.fracture_z_geometry(5) == (64, 1, 512, 128)
    assert cases.fracture_z_geometry(7) == (128, 2, 16384, 4096) and cases.fracture_z_geometry(8) == (256, 4, 65536, 4096)


def test_the_restated_walks_compute_the_min_plus():
    """first_walk + second_walk on random lines with gaps: the envelope's values are min_j f[j] + (i - j)^2 under either pop
    rule, and a wrong reload changes them"""
    rng = np.random.default_rng(2)
    wrong = 0
    for _ in range(200):
        S = int(rng.choice([8, 32, 128]))
        f = rng.integers(0, int(rng.choice([4, 100, 5000])), S).astype(np.int64)
        f[rng.random(S) < rng.choice([0.0, 0.5, 0.95])] = NONE
        c = np.arange(S, dtype=np.int64)
        brute = np.where(f == NONE, np.int64(1) << 40, f)[None, :] + (c[:, None] - c[None, :]) ** 2
        want = [NONE if v >= 1 << 40 else int(v) for v in brute.min(axis=1)]
        for strict in (False, True):
            stack, top, cascade, pops = cases.first_walk(f.tolist(), strict)
            assert cases.second_walk(f.tolist(), stack) == want
            assert top >= len(stack) and pops >= cascade and len(stack) + pops == int((f != NONE).sum())
        stack = cases.first_walk(f.tolist(), False, reload_offset=1)[0]
        wrong += cases.second_walk(f.tolist(), stack) != want
    assert wrong > 20


# ---- the references ---------------------------------------------------------------------------------------------------

def test_the_feature_transform_is_the_models_field():
    rng = np.random.default_rng(4)
    for S, density in ((32, 0.002), (32, 0.3), (64, 0.01)):
        vol = (rng.random((S, S, S)) < density).astype(np.uint8)
        for to_empty in (False, True):
            assert np.array_equal(cases.edt_reference(cases.features_of(vol, to_empty)), distance_model.field(vol, to_empty))
    assert (cases.edt_reference(np.zeros((8, 8, 8), bool)) == NONE).all()
    # z_pass: the first of the three passes
    F = rng.random((32, 32, 32)) < 0.02
    g0 = distance_model._minplus(np.where(F, np.int64(0), distance_model._INF), 2)
    assert np.array_equal(cases.z_pass(F) >= cases._FAR, g0 >= distance_model._INF)
    assert np.array_equal(cases.z_pass(F)[g0 < distance_model._INF], g0[g0 < distance_model._INF])
    g1 = distance_model._minplus(g0, 1)
    picks = np.array([0, 5, 77, 32 * 32 - 1])
    assert np.array_equal(cases.y_lines(g0, picks), cases.as_entries(np.stack([g0[l // 32, :, l % 32] for l in picks])))
    assert np.array_equal(cases.x_lines(g0, picks), cases.as_entries(np.stack([g1[:, l // 32, l % 32] for l in picks])))


def test_the_closed_form_of_the_products_is_the_feature_transform():
    for S in (32, 128):
        sets = cases.axis_sets(S)
        vol = cases.products_volume(sets)
        D = cases.products_field(sets)
        assert np.array_equal(D, cases.edt_reference(vol != 0)), S
        assert cases.product_count(sets) == int(vol.sum())
        assert cases.stats_of_finite(D) == distance_model.stats(D)
        assert np.array_equal(cases.open_border_in_place(D.copy()), distance_model.open_border(D))
        # the slabs the device volume is made of
        built = np.zeros_like(vol)
        for A, B, C in sets:
            fill, clear = cases.product_boxes(A, B, C)
            part = np.zeros_like(vol)
            for x0, y0, z0, x1, y1, z1 in fill.tolist():
                part[x0:x1, y0:y1, z0:z1] = 1
            for x0, y0, z0, x1, y1, z1 in clear.tolist():
                part[x0:x1, y0:y1, z0:z1] = 0
            built |= part
        assert np.array_equal(built, vol)
    sets = cases.axis_sets(512)
    assert len(sets) == 6 and all(X.any() for t in sets for X in t)
    first = [int(np.flatnonzero(A)[0]) for A, B, C in sets]
    assert any(A[256:].any() and B[256:].any() for A, B, C in sets) and min(first) < 256                # features in both halves


def test_the_packed_min_plus_is_the_brute_force():
    """32^3, 200 random sites with duplicates and sites outside: packed_cells is fracture_model.cells, unlimited and under cut-offs;
    the windowed form is the full one under the same cut-off"""
    S = 32
    rng = np.random.default_rng(8)
    sites = rng.integers(-2, S + 2, (200, 3))
    sites[100], sites[199], sites[50] = sites[0], sites[1], sites[0]
    P = cases.packed_field(S, sites)
    for max_d2 in (NONE, 0, 9, 16, 100):
        assert np.array_equal(cases.cells_of_packed(P, max_d2), fracture_model.cells(S, sites, max_d2)), max_d2
    for r in (0, 1, 3, 4, 8):
        assert np.array_equal(cases.packed_cells(S, sites, r * r, r), cases.cells_of_packed(P, r * r)), r
        assert np.array_equal(cases.packed_cells(S, sites, r * r - 1 if r else 0, r), cases.cells_of_packed(P, r * r - 1 if r else 0)), r
    few = sites[:12]
    for r in (0, 1, 3, 4):
        assert np.array_equal(cases.packed_cells(S, few, r * r, r), fracture_model.cells(S, few, r * r)), r
    assert (cases.packed_cells(S, few, 9, 3) == NONE).any() and (cases.packed_cells(S, sites, 1, 1) == NONE).any()
    # a regular pattern ties a lot: the lowest index, whichever order
    lattice = np.stack(np.meshgrid(*[np.arange(2, S, 6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    for order in (lattice, lattice[::-1], cases.shuffled(lattice)):
        assert np.array_equal(cases.packed_cells(S, order), fracture_model.cells(S, order))
    assert cases.tied_voxels(S, lattice, 6) > 1000


def test_the_closed_form_of_a_product_grid_is_the_packed_min_plus():
    for S, counts, triples in ((32, (5, 9, 3), 0), (64, (10, 7, 20), 0), (64, (9, 12, 2), 30), (128, (20, 30, 3), 40)):
        g = cases.grid_sites(S, counts, triples=triples)
        assert len(g.sites) == int(np.prod(counts)) + 3 * triples and not np.array_equal(g.table.reshape(-1), np.arange(g.table.size))
        want = cases.packed_cells(S, g.sites)
        assert np.array_equal(cases.grid_cells(g, S), want)
        xyz = np.concatenate([np.random.default_rng(1).integers(0, S, (500, 3)), g.centres])
        assert np.array_equal(cases.grid_cells_at(g, S, xyz), want[tuple(xyz.T)])
        if triples:
            # a voxel the tie alone gives to the middle site: the three sites are the nearest, equally near, and along the line
            # through the outer two the middle one's parabola is above one of theirs everywhere else
            won = cases.tie_won_triples(g, S)
            assert len(won) >= 3
            for t in won:
                p = g.extras[3 * t:3 * t + 3]
                d2 = ((p - g.centres[t]) ** 2).sum(axis=1)
                assert d2[0] == d2[1] == d2[2] == (p[2] - p[0]).max() ** 2 // 4
                axis = t % 2
                line = np.repeat(g.centres[t][None], S, axis=0)
                line[:, axis] = np.arange(S)
                along = ((line[:, None, :] - p[None]) ** 2).sum(axis=2)
                assert (along[:, 1] >= np.minimum(along[:, 0], along[:, 2])).all() and int((along[:, 1] == along.min(axis=1)).sum()) == 1
    for S in (256, 512):
        g = cases.grid_sites(S, cases.GRID_COUNTS[S])
        won = g.centres[cases.tie_won_triples(g, S)]
        print("%d: %d of %d triples give their centre to a middle site of lowest index" % (S, len(won), len(g.centres)))
        assert len(won) >= 5 and (S == 256 or ((won[:, 0] >= 256) | (won[:, 1] >= 256)).sum() >= 3)
        assert len(np.unique(g.sites, axis=0)) == len(g.sites)
        near = [cases.nearest_two(a, S) for a in g.axes]
        tied = [int((n[:, 0] != n[:, 1]).sum()) for n in near]
        assert all(t > 1 for t in tied), (S, tied)                      # coordinates equally near to two: ties on every axis
        assert len(g.sites) == int(np.prod(cases.GRID_COUNTS[S])) + 3 * cases.TRIPLES and g.sites.min() >= 0 and g.sites.max() < S
        if S == 512:                                                        # sites, and lines that hold some, in both steps of the line loop
            assert (g.axes[0] >= 256).sum() > 20 and (g.axes[1] >= 256).sum() > 20 and (g.axes[0] < 256).sum() > 20
            assert len(g.axes[1]) > 128 and len(g.axes[0]) > 128            # the stack depth of the y pass and of the x pass


# ---- the regimes of the walks -----------------------------------------------------------------------------------------

def lines_of(F, S, count):
    """the sampled lines of both min-plus passes over the feature set F: (y lines, x lines); a quarter as many of the x pass"""
    picks = cases.sampled_lines(S, count)
    g0 = cases.z_pass(F)
    return cases.y_lines(g0, picks), cases.x_lines(g0, picks[:max(len(picks) // 4, 1)])


def deep_and_popping(stats, S):
    return stats[(stats[:, 0] > S // 2) & (stats[:, 2] > 0)]


@pytest.mark.parametrize("strict", [False, True])
def test_slant_and_specks_at_128(strict):
    """y pass, 1024 sampled lines: a full stack, a push that pops 32 or more, and a hundred lines with both.  Under the strict
    rule the sites are the scene's voxels, so the lines are the same ones"""
    S = 128
    sites = cases.scene_sites("slant", S)
    assert len(sites) == int(cases.scene("slant", S).sum()) < cases.MAX_SITES
    y, x = lines_of(cases.scene("slant", S) != 0, S, 1024)
    stats = cases.walk_stats(y, strict)
    print("slant 128 strict %d: top %d, cascade %d, %d lines deep and popping" % (strict, stats[:, 0].max(), stats[:, 1].max(), len(deep_and_popping(stats, S))))
    assert stats[:, 0].max() == 128 and stats[:, 1].max() >= 32 and len(deep_and_popping(stats, S)) >= 100


@pytest.mark.parametrize("strict", [False, True])
def test_products_at_128(strict):
    """some line with top > 64 and a cascade of 8 or more (it is one of the x pass)"""
    S = 128
    sites = cases.scene_sites("products", S)
    assert len(sites) == int(cases.scene("products", S).sum()) < cases.MAX_SITES
    g0 = cases.z_pass(cases.scene("products", S) != 0)
    picks = np.arange(0, S * S, 4)                                          # such lines are few: every fourth line, not a sample
    stats = np.concatenate([cases.walk_stats(cases.y_lines(g0, picks), strict), cases.walk_stats(cases.x_lines(g0, picks), strict)])
    deep = stats[stats[:, 0] > S // 2]
    print("products 128 strict %d: top %d, cascade on a deep line %d" % (strict, stats[:, 0].max(), deep[:, 1].max()))
    assert deep[:, 1].max() >= 8


@pytest.mark.parametrize("name", ["slant", "ball", "products"])
def test_scenes_at_256(name):
    """in device memory: top > 128 with pops on one line, under both rules, for the solid set; the sites of the fracture are
    the scene's voxels, or whole x layers of them"""
    S = 256
    vol = cases.scene(name, S)
    y, x = lines_of(vol != 0, S, 256)
    for strict in (False, True):
        stats = np.concatenate([cases.walk_stats(y, strict), cases.walk_stats(x, strict)])
        deep = deep_and_popping(stats, S)
        print("%s 256 strict %d: top %d, %d lines deep and popping, cascade %d" % (name, strict, stats[:, 0].max(), len(deep), stats[:, 1].max()))
        assert len(deep) >= (50 if name == "ball" else 1)                    # the ball is what fills device stacks and pops on many lines
    if name != "ball":
        sites = cases.scene_sites(name, S)
        assert len(sites) <= cases.MAX_SITES and (len(sites) == int(vol.sum()) or name == "products")
        F = cases.site_set(sites, S)
        layers = np.unique(sites[:, 0])
        assert np.array_equal(F[layers], vol[layers] != 0)                    # a kept layer is the scene's


def test_the_complements_stack_to_the_full_depth():
    """to_empty: nearly every voxel is a feature with f = 0, so the stacks hold S entries; the few others pop"""
    for S, count in ((128, 256), (256, 64)):
        for name in cases.SCENES:
            y, x = lines_of(cases.scene(name, S) == 0, S, count)
            stats = cases.walk_stats(y, False)
            assert stats[:, 0].max() > S - S // 8 and len(deep_and_popping(stats, S)) >= 1, (name, S)


def test_fracture_z_pass_columns_at_256():
    """k_fracture_z carries (ci, cat) across four chunks of 64: a column with markers in all four, and one with markers in
    chunks 0 and 3 alone, so that a carry crosses two empty chunks in both directions"""
    S = 256
    seen = np.zeros(2, np.int64)
    for name in ("slant", "products"):
        chunks = cases.site_set(cases.scene_sites(name, S), S).reshape(S, S, 4, 64).any(axis=3)
        seen += [int(chunks.all(axis=2).sum()), int((chunks[:, :, 0] & chunks[:, :, 3] & ~chunks[:, :, 1] & ~chunks[:, :, 2]).sum())]
        print(name, seen)
    assert seen[0] >= 1 and seen[1] >= 1
    # and the distance field's z pass: columns with several non-empty words of its 8, and with empty words between them
    words = (cases.scene("slant", S) != 0).reshape(S, S, 8, 32).any(axis=3)
    assert int((words.sum(axis=2) >= 3).sum()) >= 1 and int((words[:, :, 0] & words[:, :, 7] & ~words[:, :, 3]).sum()) >= 1


def test_every_site_set_ties():
    """more than one voxel with several nearest sites, in every site set: the tie rule is exercised"""
    for S, window in ((128, 3), (256, 2)):
        for name in ("slant", "products"):
            tied = cases.tied_voxels(S, cases.scene_sites(name, S), window)
            print("%s %d: %d voxels within %d of a site have several nearest" % (name, S, tied, window))
            assert tied > 1


# ---- the clearance case -----------------------------------------------------------------------------------------------

def test_the_clearance_case_moves_twenty_boxes():
    S = 256
    debris, offsets = cases.clearance_case(S)
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == len(offsets) == 20
    maps = [(list(stamp_model.IDENTITY[0]), [-(int(v) << 17) for v in o]) for o in offsets]
    boxes = np.concatenate([rec["lo"].astype(np.int64) + offsets, rec["hi"].astype(np.int64) + offsets], axis=1)
    sets = posed_cases.posed_point_sets(ids, maps, boxes, S)
    for i, points in enumerate(sets):
        assert np.array_equal(points, np.argwhere(ids == i) + offsets[i]), i
    D = np.arange(S ** 3, dtype=np.uint32).reshape(S, S, S)
    rec0 = clearance_model.record(sets[0], D)
    assert rec0[0] == int(rec["voxels"][0]) and rec0[4] == [int(v) for v in rec["lo"][0]]
