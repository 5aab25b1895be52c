"""The travel-distance field on the GPU (vrc_travel_field, vrc_travel_trace_paths; VoxelVolume.travelField /
reachableWithin / shortestPath, VoxelDistance.tracePaths).  The expected field is the breadth-first model of
tests/travel_model.py (held against the definition in tests/test_volume_travel_host.py), or the analytic answer where a
test says so.  Every comparison is exact.  The device works in tiles of 16^3 voxels: depth 4 is one tile, depth 5 two per
axis, depth 6 four per axis -- the smallest with a tile that has all 26 neighbours."""

import numpy as np
import pytest

import travel_model as model
from travel_support import check_field, run_case
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu

NONE = model.NONE
TILE = 16
TRIP_BOUND = 64          # iterations of a tile in one sweep (csrc/vrc_travel.hip: TRAVEL_TILE_ITERS)


def random_seeds(rng, S, count):
    seeds = np.zeros((S, S, S), np.uint8)
    for x, y, z in rng.integers(0, S, (count, 3)):
        seeds[x, y, z] = 1
    return seeds


# ---- random volumes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_random_volumes(built, depth, connectivity):
    """Below one tile (depths 2 and 3), one tile, two and four tiles per axis; from sparse to dense, both media: near the
    percolation threshold (0.3 solid for 6 neighbours through the solid) the routes are long and winding.  1 to 20 random
    seeds, some of them outside M."""
    S = 1 << depth
    rng = np.random.default_rng(7000 + 10 * depth + connectivity)
    for density in (0.05, 0.3, 0.5, 0.7):
        vol = (rng.random((S, S, S)) < density).astype(np.uint8)
        seeds = random_seeds(rng, S, int(rng.integers(1, 21)))
        volume, seed_volume = volume_of(vol, depth), volume_of(seeds, depth)
        for through_empty in (False, True):
            run_case(vol, seeds, connectivity, through_empty, (depth, connectivity, density, through_empty), volume=volume, seed_volume=seed_volume)
        volume.close()
        seed_volume.close()


# ---- constructed cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("where", [(TILE, TILE, TILE), (TILE + 8, TILE + 8, TILE + 8)])
def test_tile_with_all_26_neighbours(built, where, connectivity):
    """Depth 6: tile (1, 1, 1) has a tile on every side.  Empty air from one seed at that tile's corner / centre: the
    Manhattan distance for 6 neighbours, the Chebyshev distance for 26."""
    depth, S = 6, 64
    d = np.abs(np.indices((S, S, S)) - np.array(where).reshape(3, 1, 1, 1))
    T = (d.sum(axis=0) if connectivity == 6 else d.max(axis=0)).astype(np.uint32)
    volume, seed_volume = volume_of(np.zeros((S, S, S), np.uint8), depth), volume_of(np.zeros((S, S, S), np.uint8), depth)
    seed_volume.setVoxels(np.array([where], np.uint32))
    field = volume.travelField(seed_volume, connectivity, through_empty=True)
    check_field(field, T, 1, connectivity, (where, connectivity))
    field.close()
    volume.close()
    seed_volume.close()


def carve(vol, corners):
    """solid voxels along the axis-aligned polyline through `corners`"""
    for a, b in zip(corners, corners[1:]):
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        vol[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = 1


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("short_first", [False, True])
def test_a_shorter_route_that_arrives_later_lowers_the_tail(built, short_first, connectivity):
    """Depth 5, corridors of solid voxels.  The seed (14, 1, 1) and the voxel P = (14, 7, 1) lie in tile 0.  One corridor
    joins them inside tile 0, one through the tile next to it in x, which runs a sweep later; behind P a tail of about 70
    voxels runs up through the tile above and back.  With the long corridor inside tile 0, P and the whole tail first get
    the long route's values and must all be lowered when the short one arrives; the mirror case has the short corridor
    inside the tile."""
    depth, S = 5, 32
    vol = np.zeros((S, S, S), np.uint8)
    seed, P = (14, 1, 1), (14, 7, 1)
    inside_long = [seed, (2, 1, 1), (2, 4, 1), (11, 4, 1), (11, 7, 1), P]                     # 12 + 3 + 9 + 3 + 3 = 30 steps, x <= 14
    outside_short = [seed, (17, 1, 1), (17, 7, 1), P]                                         # 3 + 6 + 3 = 12 steps through x >= 16
    inside_short = [seed, (13, 1, 1), (13, 7, 1), P]                                          # 1 + 6 + 1 = 8 steps
    outside_long = [seed, (17, 1, 1), (17, 4, 1), (28, 4, 1), (28, 10, 1), (17, 10, 1), (17, 7, 1), (15, 7, 1), P]
    carve(vol, inside_short if short_first else inside_long)
    carve(vol, outside_long if short_first else outside_short)
    carve(vol, [P, (14, 7, 28), (14, 20, 28), (14, 20, 3), (5, 20, 3)])                       # the tail
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[seed] = 1
    T = run_case(vol, seeds, connectivity, False, (short_first, connectivity))
    if connectivity == 6:
        assert int(T[P]) == (8 if short_first else 12) and int(T[5, 20, 3]) == int(T[P]) + 27 + 13 + 25 + 9


def serpentine(S, rows, length, z):
    """solid rows x = 0, 2, 4, ... of `length` voxels along y in the slab z, joined at alternating ends"""
    vol = np.zeros((S, S, S), np.uint8)
    for i in range(rows):
        vol[2 * i, :length, z] = 1
        if i + 1 < rows:
            vol[2 * i + 1, length - 1 if i % 2 == 0 else 0, z] = 1
    return vol


@pytest.mark.parametrize("connectivity", [6, 26])
def test_serpentine_corridor_across_many_tile_borders(built, connectivity):
    """Depth 6, one z-slab: 32 rows of 64 voxels, about 2000 steps for 6 neighbours, crossing the same tile borders dozens
    of times.  The sweeps stay within max T + 2."""
    depth, S = 6, 64
    vol = serpentine(S, 32, S, 5)
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[0, 0, 5] = 1
    T = run_case(vol, seeds, connectivity, False, ("serpentine", connectivity), with_at=False, tight=True)
    if connectivity == 6:
        assert int(T[T != NONE].max()) == 32 * 63 + 31 * 2


@pytest.mark.parametrize("connectivity", [6, 26])
def test_serpentine_inside_one_tile_longer_than_the_trip_bound(built, connectivity):
    """Depth 4 is a single tile: 8 rows of 16 voxels are 134 steps for 6 neighbours, more than twice the iterations a tile
    makes in one sweep, so the tile has to run again on its own flag.  Across the columns (x, y): a column along z is
    crossed in one iteration."""
    depth, S = 4, 16
    vol = serpentine(S, 8, S, 9)
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[0, 0, 9] = 1
    T = run_case(vol, seeds, connectivity, False, ("in one tile", connectivity), tight=True)
    if connectivity == 6:
        assert int(T[T != NONE].max()) == 8 * 15 + 7 * 2 > 2 * TRIP_BOUND


def test_two_chambers_that_touch_at_a_tile_corner(built):
    """Depth 5: the boxes [12, 16)^3 and [16, 20)^3 share only the corner where eight tiles meet: joined for 26 neighbours,
    apart for 6."""
    depth, S = 5, 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[12:16, 12:16, 12:16] = 1
    vol[16:20, 16:20, 16:20] = 1
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[12, 12, 12] = 1
    T6 = run_case(vol, seeds, 6, False, "corner, 6")
    T26 = run_case(vol, seeds, 26, False, "corner, 26")
    assert (T6[16:20, 16:20, 16:20] == NONE).all() and int(T6[15, 15, 15]) == 9
    assert int(T26[15, 15, 15]) == 3 and int(T26[16, 16, 16]) == 4 and int(T26[19, 19, 19]) == 7


# ---- step_limit ---------------------------------------------------------------------------------------------------

def test_step_limit_around_a_known_distance(built):
    depth, S = 5, 32
    vol = np.zeros((S, S, S), np.uint8)
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[3, 3, 3] = 1
    target, k = (10, 9, 10), 7 + 6 + 7
    volume, seed_volume = volume_of(vol, depth), volume_of(seeds, depth)
    for limit, want in [(k - 1, NONE), (k, k), (k + 1, k), (1, NONE), (0, k)]:
        T = run_case(vol, seeds, 6, True, ("limit", limit), step_limit=limit, volume=volume, seed_volume=seed_volume)
        assert int(T[target]) == want
        if limit == 1:
            assert int((T != NONE).sum()) == 7
    volume.close()
    seed_volume.close()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_field_under_a_limit_is_the_unlimited_field_cut_off(built, connectivity):
    depth, S = 5, 32
    rng = np.random.default_rng(7300 + connectivity)
    vol = (rng.random((S, S, S)) < 0.35).astype(np.uint8)
    seeds = random_seeds(rng, S, 6)
    volume, seed_volume = volume_of(vol, depth), volume_of(seeds, depth)
    whole = volume.travelField(seed_volume, connectivity, True)
    unlimited = whole.download()
    whole.close()
    assert np.array_equal(unlimited, model.field(vol, seeds, connectivity, True))
    for limit in (1, 2, 9, 17, int(unlimited[unlimited != NONE].max()), 1 << 30):
        field = volume.travelField(seed_volume, connectivity, True, limit)
        assert np.array_equal(field.download(), np.where(unlimited > limit, NONE, unlimited)), limit
        assert int(field.stats.sweeps) <= limit + 2
        field.close()
    volume.close()
    seed_volume.close()


# ---- degenerate inputs ----------------------------------------------------------------------------------------------

def test_degenerate_inputs(built):
    depth, S = 5, 32
    rng = np.random.default_rng(7400)
    vol = (rng.random((S, S, S)) < 0.4).astype(np.uint8)
    none, full = np.zeros((S, S, S), np.uint8), np.ones((S, S, S), np.uint8)
    some = random_seeds(rng, S, 12)
    T = run_case(vol, none, 6, False, "no seeds")
    assert (T == NONE).all()
    T = run_case(vol, (some != 0) & (vol == 0), 26, False, "all seeds outside M")
    assert (T == NONE).all()
    T = run_case(none, some, 6, False, "M empty")
    assert (T == NONE).all()
    T = run_case(full, full, 26, True, "M empty, through the empty voxels of a full volume")
    assert (T == NONE).all()
    run_case(full, some, 6, False, "M the whole volume")
    run_case(none, some, 26, True, "M the whole volume, through the air")
    corners = np.zeros((S, S, S), np.uint8)
    for x in (0, S - 1):
        for y in (0, S - 1):
            for z in (0, S - 1):
                corners[x, y, z] = 1
    T = run_case(none, corners, 6, True, "eight corners")
    assert int(T.max()) == 3 * 15 and int(T[0, 0, 1]) == 1 and int(T[0, 0, S - 2]) == 1      # walls: no way round through a face
    T = run_case(none, corners, 26, True, "eight corners, 26")
    assert int(T.max()) == 15
    # seeds is medium: every solid voxel is a seed
    volume = volume_of(vol, depth)
    field = volume.travelField(volume, 6)
    check_field(field, np.where(vol != 0, 0, NONE).astype(np.uint32), int(vol.sum()), 6, "seeds is medium")
    field.close()
    field = volume.travelField(volume, 26, through_empty=True)
    check_field(field, np.full((S, S, S), NONE, np.uint32), 0, 26, "seeds is medium, through the air")
    field.close()
    volume.close()


# ---- identical bytes, snapshots ---------------------------------------------------------------------------------------

def test_identical_bytes_and_snapshot_lifetime(built):
    depth, S = 5, 32
    rng = np.random.default_rng(7500)
    vol = (rng.random((S, S, S)) < 0.6).astype(np.uint8)
    seeds = random_seeds(rng, S, 5)
    seeds[vol == 0] = 0
    seeds[np.unravel_index(np.flatnonzero(vol)[0], vol.shape)] = 1
    volume, seed_volume = volume_of(vol, depth), volume_of(seeds, depth)
    scratch = volume.editScratchBytes(), seed_volume.editScratchBytes()
    first = volume.travelField(seed_volume, 26)
    second = volume.travelField(seed_volume, 26)
    assert (volume.editScratchBytes(), seed_volume.editScratchBytes()) == scratch       # all scratch is freed
    a = first.download()
    assert a.tobytes() == second.download().tobytes() and np.array_equal(a, model.field(vol, seeds, 26, False))
    second.close()
    wall = np.zeros((S, S, S), np.uint8)
    wall[S // 2] = 1
    volume.fillBoxes([[S // 2, 0, 0, S // 2 + 1, S, S]], solid=False)          # an edit of the medium: a gap across the volume
    third = volume.travelField(seed_volume, 26)
    b = third.download()
    assert np.array_equal(b, model.field(vol & ~wall, seeds, 26, False)) and not np.array_equal(a, b)
    third.close()
    volume.close()
    seed_volume.close()
    assert np.array_equal(first.download(), a) and first.connectivity == 26            # outlives both volumes, unchanged
    first.close()


# ---- select and reachability ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cave(built):
    """one depth-6 case shared by the select and the route tests: (vol, seeds, connectivity, T of the model)"""
    S = 64
    rng = np.random.default_rng(7600)
    vol = (rng.random((S, S, S)) < 0.36).astype(np.uint8)             # just above the threshold: one winding piece holds most
    seeds = random_seeds(rng, S, 2)                                   # anywhere: most likely outside M
    for x, y, z in np.argwhere(vol)[rng.choice(int(vol.sum()), 6, replace=False)]:
        seeds[x, y, z] = 1
    return vol, seeds, 6, model.field(vol, seeds, 6, False)


def test_select_and_reachability(cave):
    import cpuvoxelraycaster_amd as vrc
    capi = vrc.capi
    vol, seeds, connectivity, T = cave
    depth, S = 6, 64
    volume, seed_volume = volume_of(vol, depth), volume_of(seeds, depth)
    field = volume.travelField(seed_volume, connectivity)
    k = 11
    near = model.select(T, 0, k)
    other = (np.random.default_rng(7601).random((S, S, S)) < 0.5)
    for op, want in [(capi.VRC_COPY_REPLACE, near), (capi.VRC_COPY_OR, other | near), (capi.VRC_COPY_ANDNOT, other & ~near)]:
        dst = volume_of(other, depth)
        field.select(0, k, dst, op)
        assert np.array_equal(dst.download() != 0, want), op
        dst.close()
    never = field.select(NONE, NONE)
    assert np.array_equal(never.download() != 0, T == NONE)
    never.close()
    within = volume.reachableWithin(seed_volume, k, connectivity)
    assert np.array_equal(within.download() != 0, near)
    within.close()
    at_once = volume.reachableWithin(seed_volume, 0, connectivity)
    assert np.array_equal(at_once.download() != 0, T == 0)
    at_once.close()
    # every voxel with a value is what the flood reaches from the same seeds in the same medium, and nothing else
    everything = field.select(0, NONE - 1)
    flooded = seed_volume.clone()
    st = flooded.flood(volume, connectivity)
    assert st.converged == 1 and int(st.reached) == int(field.stats.reached)
    assert np.array_equal(everything.download(), flooded.download()) and np.array_equal(flooded.download() != 0, T != NONE)
    for v in (everything, flooded, field, volume, seed_volume):
        v.close()


# ---- routes -------------------------------------------------------------------------------------------------------

def check_routes_by_property(routes, lengths, starts, T, M, connectivity):
    for start, length, route in zip(starts, lengths, routes):
        length = int(length)
        if length == NONE:
            assert len(route) == 0
            continue
        assert len(route) == length + 1 and tuple(route[0]) == tuple(start)
        r = route.astype(np.int64)
        step = np.abs(np.diff(r, axis=0))
        assert (step.max(axis=1) == 1).all() if len(step) else True
        if connectivity == 6 and len(step):
            assert (step.sum(axis=1) == 1).all()
        values = T[r[:, 0], r[:, 1], r[:, 2]]
        assert np.array_equal(values, np.arange(length, -1, -1)) and M[r[:, 0], r[:, 1], r[:, 2]].all() and values[-1] == 0


@pytest.mark.parametrize("connectivity", [6, 26])
def test_routes_from_every_reachable_voxel_at_depth_4(built, connectivity):
    depth, S = 4, 16
    rng = np.random.default_rng(7700 + connectivity)
    vol = (rng.random((S, S, S)) < 0.45).astype(np.uint8)
    seeds = random_seeds(rng, S, 3)
    T = model.field(vol, seeds, connectivity, False)
    volume, seed_volume = volume_of(vol, depth), volume_of(seeds, depth)
    field = volume.travelField(seed_volume, connectivity)
    starts = np.concatenate([np.argwhere(T != NONE), np.argwhere(T == NONE)[:5], [[S, 0, 0], [0, 0, 0xFFFFFFFF]]]).astype(np.uint32)
    lengths, routes = field.tracePaths(starts)
    want = [model.trace(T, s, connectivity) for s in starts]
    assert np.array_equal(lengths, np.array([w[0] for w in want], np.uint32))
    for got, (_, route) in zip(routes, want):
        assert np.array_equal(got, route)
    check_routes_by_property(routes, lengths, starts, T, vol != 0, connectivity)
    for v in (field, volume, seed_volume):
        v.close()


def test_routes_at_depth_6_capacity_and_device_memory(cave):
    import torch
    vol, seeds, connectivity, T = cave
    depth, S = 6, 64
    rng = np.random.default_rng(7800)
    volume, seed_volume = volume_of(vol, depth), volume_of(seeds, depth)
    field = volume.travelField(seed_volume, connectivity)
    reachable = np.argwhere(T != NONE)
    starts = np.concatenate([reachable[rng.choice(len(reachable), 246, replace=False)], np.argwhere(T == 0)[:2], np.argwhere(T == 2)[:2],
                             np.argwhere(T == NONE)[:4], [[0, S, 0], [S + 3, 1, 1]]]).astype(np.uint32)       # routes of 0 and 2 steps among them
    assert len(starts) == 256
    lengths, routes = field.tracePaths(starts)
    want = [model.trace(T, s, connectivity) for s in starts]
    assert np.array_equal(lengths, np.array([w[0] for w in want], np.uint32))
    for got, (_, route) in zip(routes, want):
        assert np.array_equal(got, route)
    check_routes_by_property(routes, lengths, starts, T, vol != 0, connectivity)

    # a capacity below the longest route truncates it; what lies behind a route's end, and the rows of starts without a
    # value, keep their sentinel
    import cpuvoxelraycaster_amd as vrc
    capi, L = vrc.capi, vrc.capi.load()
    capacity, sentinel = 6, 0xABABABAB
    paths = np.full((len(starts), capacity, 3), sentinel, np.uint32)
    got_lengths = np.full(len(starts), sentinel, np.uint32)
    capi.check(L.vrc_travel_trace_paths(field._h, len(starts), capi.ptr(starts), capacity, capi.ptr(paths), capi.ptr(got_lengths), capi.VRC_MEM_HOST, None))
    assert np.array_equal(got_lengths, lengths) and (lengths[lengths != NONE] >= capacity).any() and (lengths < capacity - 1).any()
    for i, (length, route) in enumerate(want):
        k = 0 if length == NONE else min(length, capacity - 1) + 1
        assert np.array_equal(paths[i, :k], route[:k]) and (paths[i, k:] == sentinel).all(), i
    cut_lengths, cut = field.tracePaths(starts, capacity)
    assert np.array_equal(cut_lengths, lengths) and all(np.array_equal(c, w[1][:capacity]) for c, w in zip(cut, want))
    # capacity 0 without a buffer: the lengths alone
    got_lengths[:] = sentinel
    capi.check(L.vrc_travel_trace_paths(field._h, len(starts), capi.ptr(starts), 0, None, capi.ptr(got_lengths), capi.VRC_MEM_HOST, None))
    assert np.array_equal(got_lengths, lengths)

    # device memory, on a stream
    d_starts = torch.from_numpy(starts.astype(np.int64)).to(torch.int32).cuda()       # the same 32 bits
    d_paths = torch.full((len(starts), capacity, 3), -1, dtype=torch.int32, device="cuda")
    d_lengths = torch.full((len(starts),), -2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with Stream() as stream:
        field.tracePathsDevice(len(starts), d_starts.data_ptr(), capacity, d_paths.data_ptr(), d_lengths.data_ptr(), stream)
    assert np.array_equal(d_lengths.cpu().numpy().view(np.uint32), lengths)
    on_device = d_paths.cpu().numpy().view(np.uint32)
    assert np.array_equal(np.where(paths == sentinel, 0xFFFFFFFF, paths), on_device)
    for v in (field, volume, seed_volume):
        v.close()


def test_routes_are_refused_on_a_euclidean_field(built):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(4)
    volume.setVoxels([[3, 3, 3]])
    euclid = volume.distanceField()
    assert euclid.connectivity == 0
    with pytest.raises(vrc.VrcError, match="vrc_travel_trace_paths: not a travel field"):
        euclid.tracePaths([[1, 1, 1]])
    euclid.close()
    volume.close()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_shortest_path(built, connectivity):
    """Through the air of a depth-5 volume with a wall that has one door; None across a wall without one."""
    depth, S = 5, 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[15] = 1
    vol[15, 20, 7] = 0
    a, b = (3, 4, 5), (29, 10, 25)
    volume = volume_of(vol, depth)
    route = volume.shortestPath(a, b, connectivity)
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[b] = 1
    T = model.field(vol, seeds, connectivity, True)
    assert route.shape == (int(T[a]) + 1, 3) and tuple(route[0]) == a and tuple(route[-1]) == b
    assert np.array_equal(route, model.trace(T, a, connectivity)[1])
    check_routes_by_property([route], [int(T[a])], [a], T, vol == 0, connectivity)
    assert (route == (15, 20, 7)).all(axis=1).any()                 # through the door
    volume.fillBoxes([[15, 20, 7, 16, 21, 8]])
    assert volume.shortestPath(a, b, connectivity) is None
    assert volume.shortestPath(a, (15, 3, 3), connectivity) is None            # b inside the wall: no seed in M
    solid = volume.shortestPath((15, 0, 0), (15, 31, 31), connectivity, through_empty=False)
    assert len(solid) == (63 if connectivity == 6 else 32)
    volume.close()
