"""The two sweep-scheme kernels of the voxel volume, the travel-distance field (csrc/vrc_travel.hip) and the flood fill
(csrc/vrc_flood.hip), at 256^3: k_travel_stats under its cap of 4096 workgroups, every lane taking four quads; sweeps of
4096 and 512 workgroups, far more than start together, over hundreds of sweeps in batches of eight; routes of more than
20000 steps.  The scenes, the geometry they reach and the expected results are tests/sweep_cases.py's, held to their
conditions in tests/test_volume_sweep_cases_host.py; the expected values come from travel_model and flood_model, never from
another GPU result, and every comparison is exact.  Each test prints the sweeps the device issued and the time its calls
took; nothing asserts a time, and the sweeps are held only from above (max T + 2, step_limit + 2): from below they depend on
the order in which the device runs the tiles."""
import time

import numpy as np
import pytest

import sweep_cases as cases
import travel_model as model
from travel_support import check_field
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu
NONE = cases.NONE


@pytest.fixture(scope="module")
def device(built):
    """name -> (the scene's volume, its seeds as a volume), uploaded once"""
    made = {}

    def get(name):
        if name not in made:
            s = cases.scene(name)
            made[name] = (volume_of(s.vol, s.depth), volume_of(s.seeds, s.depth))
        return made[name]

    yield get
    for pair in made.values():
        for v in pair:
            v.close()


def same(got, want, what):
    """np.array_equal, with the first few differing coordinates in the message"""
    if not np.array_equal(got, want):
        where = np.argwhere(got != want)
        raise AssertionError("%s: %d voxels differ, the first at %s" % (what, len(where), where[:5].tolist()))


# ---- the travel field ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,connectivity", cases.CASES)
def test_travel_field(device, name, connectivity):
    """the whole field, the stats (seeds, reached, max_steps, the farthest voxel), sweeps <= max T + 2, at() on a sample,
    select over the middle third of the values; all scratch is freed"""
    s = cases.scene(name)
    T = cases.expected_field(name, connectivity)
    volume, seed_volume = device(name)
    scratch = (volume.editScratchBytes(), seed_volume.editScratchBytes())
    start = time.perf_counter()
    field = volume.travelField(seed_volume, connectivity, s.through_empty)
    took = time.perf_counter() - start
    assert (volume.editScratchBytes(), seed_volume.editScratchBytes()) == scratch       # travel_scratch_bytes are freed again
    st = field.stats
    print("%s, %d neighbours: %d sweeps for %d steps at most (the synchronous schedule: %d), %d reached, travelField %.1f ms"
          % (name, connectivity, st.sweeps, st.max_steps, s.sweeps_implied(connectivity), st.reached, 1e3 * took))
    check_field(field, T, cases.n_seeds(name), connectivity, (name, connectivity), with_at=False, tight=True)
    xyz = cases.sample_coordinates(T, 8000 + connectivity)
    assert np.array_equal(field.at(xyz), T[tuple(xyz.astype(np.int64).T)]), (name, connectivity)
    m = int(st.max_steps)
    lo, hi = m // 3, 2 * m // 3
    band = field.select(lo, hi)
    got = band.download()
    band.close()
    field.close()
    want = model.select(T, lo, hi)
    assert 0 < int(want.sum()) < int((T != NONE).sum())
    same(got != 0, want, ("select", name, connectivity))


def border_voxel(name):
    """a voxel just beyond a tile border, some way from the seed"""
    if name == "slab_corner":
        return (16, 16, 126)
    rows, ya, yb, z = cases.SERPENTINES[name[len("serpentine_"):]]
    return (16, ya, z)                       # the first voxel of the ninth row: the first in the second plane of tiles


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", ["slab_corner", "serpentine_rows"])
def test_travel_field_under_a_step_limit(device, name, connectivity):
    """one limit below and one above the distance of a voxel behind a tile border: the unlimited field cut off at the limit,
    within limit + 2 sweeps"""
    s = cases.scene(name)
    unlimited = cases.expected_field(name, connectivity)
    p = border_voxel(name)
    d = int(unlimited[p])
    assert d != NONE and d > 2 and int(cases.travel_tile_of(p, s.S)) != int(cases.travel_tile_of(np.argwhere(s.seeds)[0], s.S))
    volume, seed_volume = device(name)
    for limit in (d - 1, d + 1):
        T = np.where(unlimited > limit, NONE, unlimited).astype(np.uint32)
        assert int(T[p]) == (NONE if limit < d else d)
        field = volume.travelField(seed_volume, connectivity, s.through_empty, limit)
        print("%s, %d neighbours, limit %d: %d sweeps" % (name, connectivity, limit, field.stats.sweeps))
        check_field(field, T, cases.n_seeds(name), connectivity, (name, connectivity, limit), step_limit=limit, with_at=False)
        assert int(field.stats.sweeps) <= limit + 2 and int(field.stats.max_steps) == limit
        field.close()


# ---- routes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", ["serpentine_rows", "serpentine_corners"])
def test_routes_along_the_serpentine(device, name, connectivity):
    """from the far end with room for the whole route, cut at 4096 voxels, and 256 starts along the corridor in device memory"""
    import torch
    s = cases.scene(name)
    T = cases.expected_field(name, connectivity)
    length, route = cases.expected_route(name, connectivity)
    far = cases.far_end(name)
    assert length >= 20000 and len(route) == length + 1 and tuple(route[-1]) == tuple(np.argwhere(s.seeds)[0])
    volume, seed_volume = device(name)
    field = volume.travelField(seed_volume, connectivity)
    start = time.perf_counter()
    lengths, routes = field.tracePaths([far], length + 1)
    took = time.perf_counter() - start
    print("%s, %d neighbours: a route of %d steps traced in %.1f ms" % (name, connectivity, length, 1e3 * took))
    assert int(lengths[0]) == length
    same(routes[0], route, ("route", name, connectivity))
    lengths, routes = field.tracePaths([far], 4096)
    assert int(lengths[0]) == length and routes[0].shape == (4096, 3)
    same(routes[0], route[:4096], ("route cut at 4096", name, connectivity))

    # 256 starts spread along the corridor, 64 voxels of each route, in device memory on a stream
    capacity = 64
    starts = route[np.linspace(0, length, 256).astype(np.int64)].astype(np.uint32)
    want = [model.trace(T, p, connectivity, capacity) for p in starts]
    d_starts = torch.from_numpy(starts.astype(np.int64)).to(torch.int32).cuda()
    d_paths = torch.full((len(starts), capacity, 3), -1, dtype=torch.int32, device="cuda")
    d_lengths = torch.full((len(starts),), -2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with Stream() as stream:
        field.tracePathsDevice(len(starts), d_starts.data_ptr(), capacity, d_paths.data_ptr(), d_lengths.data_ptr(), stream)
    got_lengths = d_lengths.cpu().numpy().view(np.uint32)
    got_paths = d_paths.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_lengths, np.array([w[0] for w in want], np.uint32))
    assert got_lengths[0] == length and got_lengths[-1] == 0 and len(set(got_lengths.tolist())) == 256
    for i, (steps, part) in enumerate(want):
        k = min(steps, capacity - 1) + 1
        assert np.array_equal(got_paths[i, :k], part) and (got_paths[i, k:] == 0xFFFFFFFF).all(), i
    field.close()


# ---- the flood ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,connectivity", cases.CASES)
def test_flood(device, name, connectivity):
    """the region against flood_model and against the travel field's reached set; the scratch grows by flood_scratch_bytes;
    capped at half the sweeps the full run issued it reports a partial result between the seeds and the answer"""
    s = cases.scene(name)
    want = cases.expected_region(name, connectivity)
    volume, seed_volume = device(name)
    region = seed_volume.clone()
    before = region.editScratchBytes()
    start = time.perf_counter()
    st = region.flood(volume, connectivity, s.through_empty)
    took = time.perf_counter() - start
    print("%s, %d neighbours: flood in %d sweeps, %d reached, %.1f ms" % (name, connectivity, st.sweeps, st.reached, 1e3 * took))
    assert region.editScratchBytes() == before + cases.flood_scratch_bytes(s.depth)
    assert st.converged == 1 and 2 <= st.sweeps <= 8 ** s.depth + 1
    got = region.download()
    same(got, want, ("flood", name, connectivity))
    assert st.reached == int(want.sum(dtype=np.int64)) == region.solidCount()

    field = volume.travelField(seed_volume, connectivity, s.through_empty)
    everything = field.select(0, NONE - 1)
    assert int(field.stats.reached) == st.reached
    same(everything.download(), got, ("the travel field's reached set", name, connectivity))
    everything.close()
    field.close()
    region.close()

    half = int(st.sweeps) // 2
    capped = seed_volume.clone()
    cut = capped.flood(volume, connectivity, s.through_empty, half)
    part = capped.download()
    capped.close()
    assert cut.converged == 0 and cut.sweeps == half, (name, connectivity, int(st.sweeps), int(cut.sweeps), int(cut.converged))
    in_m = model.seeds_in_m(s.vol, s.seeds, s.through_empty)
    assert part[in_m].all() and not np.any(part > want) and int(part.sum(dtype=np.int64)) == cut.reached < st.reached
