"""The cases of tests/test_gpu_volume_sweep_large.py without a GPU (tests/sweep_cases.py): the geometry restated there puts
k_travel_stats under its cap of 4096 workgroups with four quads a lane at 256^3; the later quads hold what decides the result
(a loop that drops them is told apart in every scene); the farthest voxel lies in the quarter of x it is meant for; the
corridors force enough changes of tile that the host loop passes its first three batches, the serpentines many hundreds; and
the two models agree on what is reached.  If the restated geometry stops matching the code, update the restatement; the
conditions stay."""
import time

import numpy as np
import pytest

import sweep_cases as cases
import travel_model

NONE = cases.NONE
FIRST_BATCHES = 2 + 4 + 8


# ---- the restated geometry --------------------------------------------------------------------------------------------

def test_restated_geometry():
    assert [cases.travel_tiles_per_axis(S) for S in (4, 8, 16, 32, 64, 128, 256)] == [1, 1, 1, 2, 4, 8, 16]
    assert [cases.flood_tiles_per_axis(S) for S in (4, 16, 32, 64, 128, 256)] == [1, 1, 1, 2, 4, 8]
    assert cases.travel_tile_of((255, 255, 255), 256) == 4095 and cases.travel_tile_of((16, 15, 32), 256) == 256 + 2
    assert cases.flood_tile_of((255, 255, 255), 256) == 511 and cases.flood_tile_of((32, 31, 64), 256) == 64 + 2
    tiles = np.arange(4096)
    tx, ty, tz = cases.tile_split(tiles, 16)
    assert np.array_equal((tx * 16 + ty) * 16 + tz, tiles) and tx.max() == ty.max() == tz.max() == 15
    xyz = np.random.default_rng(1).integers(0, 256, (1000, 3))
    for tile_of, T, edge in ((cases.travel_tile_of, 16, 16), (cases.flood_tile_of, 8, 32)):
        split = np.stack(cases.tile_split(tile_of(xyz, 256), T), axis=1)
        assert np.array_equal(split, xyz // edge)
    # the stats launch: the cap first binds at 256^3
    assert [cases.stats_launch(d) for d in (2, 6, 7, 8, 9)] == [(16, 1), (1 << 16, 256), (1 << 19, 2048), (1 << 22, 4096), (1 << 25, 4096)]
    assert [cases.quads_per_lane(d) for d in (6, 7, 8, 9)] == [1, 1, 4, 32]
    assert cases.stats_lane((0, 0, 0), 256, 4096) == (0, 0, 0) and cases.stats_lane((64, 0, 4), 256, 4096) == (1, 0, 1)
    assert cases.stats_lane((255, 255, 255), 256, 4096) == (3, 4095, 255)
    # the host loop's batches
    assert cases.batches(1) == [2] and cases.batches(3) == [2, 4] and cases.batches(7) == [2, 4, 8] and cases.batches(14) == [2, 4, 8]
    assert cases.batches(15) == [2, 4, 8, 8] and sum(cases.batches(1211)) == 1214
    assert cases.batches(100, 17) == [2, 4, 8, 3] and cases.batches(100, 1) == [1] and cases.batches(2, 17) == [2]
    assert cases.travel_scratch_bytes(8) == 24 + (3 * 4096 + 8) * 4 and cases.flood_scratch_bytes(8) == (3 * 512 + 8) * 4
    assert cases.travel_scratch_bytes(3) == 24 + 11 * 4 and cases.flood_scratch_bytes(4) == 11 * 4


def test_stats_pass_on_a_small_field():
    """stats_pass against travel_model.stats on a random field with ties, under launches of 1 to 4 quads a lane; what the two
    wrong variants get wrong"""
    rng = np.random.default_rng(2)
    T = rng.integers(0, 40, (32, 32, 32)).astype(np.uint32)
    T[rng.random(T.shape) < 0.5] = NONE
    assert int((T == 39).sum()) > 4
    for groups in (32, 16, 8):                                  # 8192 quads: 1, 2 and 4 a lane
        assert cases.stats_pass(T, groups) == travel_model.stats(T, 0)[1:]
    reached, m, arg = cases.stats_pass(T, 8, drop_later=True)
    assert reached == int((T[:8] != NONE).sum()) and arg[0] < 8
    assert cases.stats_pass(np.full((8, 8, 8), NONE, np.uint32), 1) == (0, 0, (0, 0, 0))
    by_lane = cases.stats_pass(T, 8, tie="lane")
    assert by_lane[:2] == cases.stats_pass(T, 8)[:2] and int(T[by_lane[2]]) == 39


def test_polyline_and_routes():
    voxels, turn = cases.polyline([(0, 5, 1), (3, 5, 1), (3, 7, 1), (1, 7, 1)])
    assert voxels.tolist() == [[0, 5, 1], [1, 5, 1], [2, 5, 1], [3, 5, 1], [3, 6, 1], [3, 7, 1], [2, 7, 1], [1, 7, 1]]
    assert turn.tolist() == [False, False, False, True, False, True, False, False]
    assert cases.route_of((voxels, turn), 26).tolist() == [[0, 5, 1], [1, 5, 1], [2, 5, 1], [3, 6, 1], [2, 7, 1], [1, 7, 1]]
    assert cases.crossings(np.array([[14, 16, 0], [15, 15, 0], [16, 16, 0]]), 256) == 2
    assert cases.tile_distance((0, 0, 0), (255, 40, 17), 6) == 15 + 2 + 1 and cases.tile_distance((0, 0, 0), (255, 40, 17), 26) == 15


# ---- the scenes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,connectivity", cases.CASES)
def test_scene_is_in_its_regime(name, connectivity):
    s = cases.scene(name)
    S = s.S
    start = time.perf_counter()
    T = cases.expected_field(name, connectivity)
    field_s = time.perf_counter() - start
    start = time.perf_counter()
    R = cases.expected_region(name, connectivity)
    flood_s = time.perf_counter() - start
    seeds, reached, m, arg = travel_model.stats(T, cases.n_seeds(name))
    print("%s, %d neighbours: %d reached, %d steps at most at %s, %d sweeps implied; models %.2f s and %.2f s (0 = made before)"
          % (name, connectivity, reached, m, arg, s.sweeps_implied(connectivity), field_s, flood_s))
    assert 0 < seeds and 0 < reached < 2.1e6
    # the two models agree on what is reached
    assert np.array_equal(T != NONE, R != 0)
    # the stats pass as the kernel combines it
    quads, groups = cases.stats_launch(s.depth)
    assert cases.stats_pass(T, groups) == (reached, m, arg)
    dropped = cases.stats_pass(T, groups, drop_later=True)
    if name in cases.LARGE:
        assert s.depth == 8 and groups == cases.STATS_GROUPS_MAX < (quads + cases.GROUP - 1) // cases.GROUP and cases.quads_per_lane(s.depth) == 4
        assert dropped[0] != reached
        per_quarter = [int((T[64 * q:64 * q + 64] != NONE).sum()) for q in range(4)]
        assert dropped[0] == per_quarter[0] and sum(per_quarter) == reached
    else:
        assert s.depth == 7 and groups == 2048 and cases.quads_per_lane(s.depth) == 1 and dropped == (reached, m, arg)
    if s.quarter is not None:
        assert arg[0] // 64 == s.quarter == cases.stats_lane(arg, S, groups)[0]
        if s.quarter >= 1:
            assert dropped[1:] != (m, arg)
    if name.startswith("quarters"):
        assert len(set(per_quarter)) == 4 and min(per_quarter) > 0, per_quarter
    if name.startswith("ties"):
        ends = [tuple(p[0][-1].tolist()) for p in s.paths]
        assert len({int(T[e]) for e in ends}) == 1 and int(T[ends[0]]) == m and len({e[0] // 64 for e in ends}) == len(ends)
        assert arg == min(ends) and min(ends)[0] >= 64
    # the corridors' routes as restated are shortest routes: the model's values along them count up from 0
    for path in s.paths or []:
        route = cases.route_of(path, connectivity)
        assert np.array_equal(T[tuple(route.T)], np.arange(len(route)))
    # sweeps: beyond the first three batches, so that batches of eight and the reset of the counters are reached
    implied = s.sweeps_implied(connectivity)
    assert implied > FIRST_BATCHES and implied <= m + 2
    b = cases.batches(implied)
    assert b[:4] == [2, 4, 8, 8] and len(b) - 1 >= 3
    if name.startswith("serpentine"):
        assert implied > 500 and m >= 20000
        assert m == int(T[cases.far_end(name)]) and arg == cases.far_end(name)


def test_the_chosen_pair_of_ties():
    """ties_lanes: both ends in one workgroup of the stats pass, the winner under thread 255 in the lane's second quad, the
    loser under thread 0 in its third; a combine that breaks the tie by thread takes the loser"""
    s = cases.scene("ties_lanes")
    groups = cases.stats_launch(8)[1]
    winner, loser = [tuple(p[0][-1].tolist()) for p in s.paths]
    assert cases.stats_lane(winner, 256, groups) == (1, 16 * 64 + 10, 255)
    assert cases.stats_lane(loser, 256, groups) == (2, 16 * 64 + 10, 0)
    for connectivity in (6, 26):
        T = cases.expected_field("ties_lanes", connectivity)
        assert T[winner] == T[loser] == T[T != NONE].max()
        assert cases.stats_pass(T, groups)[2] == winner and cases.stats_pass(T, groups, tie="lane")[2] == loser


def test_corner_turns_of_the_second_serpentine():
    """serpentine_corners: every turn lies on a tile border in y, those at x = 15 mod 16 on a corner of travel tiles (at x = 31 mod 32: of flood tiles too), where the route of 26
    neighbours steps diagonally through three tiles"""
    s = cases.scene("serpentine_corners")
    voxels, turn = s.paths[0]
    assert set((voxels[turn][:, 1] % 32).tolist()) == {31, 0} and turn.sum() == 2 * 104
    route = cases.route_of(s.paths[0], 26)
    at = {tuple(v): i for i, v in enumerate(route.tolist())}
    z = cases.SERPENTINES["corners"][3]
    found = 0
    for x in range(15, 208, 16):
        i = at[(x, 31, z)]
        three = route[i - 1:i + 2]
        assert three.tolist() == [[x - 1, 32, z], [x, 31, z], [x + 1, 32, z]]
        assert len(set(cases.travel_tile_of(three, 256).tolist())) == 3
        found += len(set(cases.flood_tile_of(three, 256).tolist())) == 3
    assert found == 6                                           # x = 31, 63, 95, 127, 159, 191


def test_scenes_together_cover_the_tiles():
    """more than 1024 different travel tiles hold a reached voxel in the 256^3 scenes taken together, in every plane tile / (T T);
    the slab's frontier alone crosses 256 or more tiles in each of its two planes"""
    seen = set()
    for name in cases.LARGE:
        T = cases.expected_field(name, 6)
        tiles = np.unique(cases.travel_tile_of(np.argwhere(T != NONE), 256))
        if name == "slab_corner":
            tx, ty, tz = cases.tile_split(tiles, 16)
            assert int(((tz == 7) | (tz == 8)).sum()) == 512 and int(((tx == 7) | (tx == 8)).sum()) == 512 and len(tiles) == 960
        seen |= set(tiles.tolist())
    assert len(seen) > 1024, len(seen)
    assert set(cases.tile_split(np.array(sorted(seen)), 16)[0].tolist()) == set(range(16))
    air = cases.expected_field("air128", 6)
    assert len(np.unique(cases.travel_tile_of(np.argwhere(air != NONE), 128))) == 512
