"""vrc_volume_flood on a machine without a GPU: the refusals that need no device, the C++ host adapter with
HipVoxelVolume::flood / keepConnected under a plain C++14 compiler, and the yardstick of the GPU tests itself -- the
numpy model of tests/flood_model.py against a plain breadth-first search."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest

import flood_model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flood_refusals_need_no_gpu(built):
    """Null pointers, the same volume twice, a connectivity other than 6 / 26 and a `through` other than 0 / 1 are refused
    with VRC_ERR_INVALID and the function's name before any HIP call -- and before either volume is read: with a bad
    connectivity or `through` the two handles here are not volumes at all."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    assert capi.VRC_CONNECT_FACES == 6 and capi.VRC_CONNECT_ALL == 26 and capi.VRC_FLOOD_SOLID == 0 and capi.VRC_FLOOD_EMPTY == 1
    assert C.sizeof(capi.FloodStats) == 16
    a, b = (C.c_uint64 * 64)(), (C.c_uint64 * 64)()          # 512 bytes each of something that is not a vrc_volume
    pa, pb = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    st = capi.FloodStats(reached=7, sweeps=7, converged=7)
    cases = [
        (None, None, 6, 0), (None, pb, 6, 0), (pa, None, 26, 1),      # null pointers
        (pa, pa, 6, 0),                                               # the same volume twice
        (pa, pb, 0, 0), (pa, pb, 18, 0), (pa, pb, -6, 1), (pa, pb, 27, 0),
        (pa, pb, 6, 2), (pa, pb, 26, -1),
    ]
    for region, medium, conn, through in cases:
        for stats in (None, C.byref(st)):
            assert L.vrc_volume_flood(region, medium, conn, through, 0, stats) == -1, (conn, through)
            assert L.vrc_last_error().startswith(b"vrc_volume_flood"), L.vrc_last_error()
    assert (st.reached, st.sweeps, st.converged) == (7, 7, 7)         # nothing was written
    assert not any(a) and not any(b)


def test_host_adapter_with_flood_compiles(built):
    """HipVoxelVolume::flood / keepConnected in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world) {\n'
           '    vrc_host::HipVoxelVolume region(world.depth());\n'
           '    region.fillBox(0, 0, 0, 4, 4, 4, true);\n'
           '    vrc_flood_stats a = region.flood(world);\n'
           '    vrc_flood_stats b = region.flood(world, VRC_CONNECT_ALL, true, 3);\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> debris = world.keepConnected({0, 0, 0, 8, 1, 8});\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> more = world.keepConnected({0, 0, 0, 8, 1, 8}, VRC_CONNECT_ALL);\n'
           '    return a.reached + b.sweeps + b.converged + debris->solidCount() + more->solidCount();\n'
           '}\nint main(){ return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
    main = os.path.join(ROOT, "tests", "cpp", "voxel_flood_main.cpp")
    check_cpp_syntax(main, strict=True)


def bfs(M, seeds, connectivity):
    S = M.shape[0]
    steps = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    assert len(steps) == connectivity
    out = np.zeros(M.shape, np.uint8)
    queue = deque()
    for p in map(tuple, np.argwhere(seeds)):
        if M[p]:
            out[p] = 1
            queue.append(p)
    while queue:
        x, y, z = queue.popleft()
        for dx, dy, dz in steps:
            q = (x + dx, y + dy, z + dz)
            if min(q) < 0 or max(q) >= S or out[q] or not M[q]:
                continue
            out[q] = 1
            queue.append(q)
    return out


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("through_empty", [False, True])
def test_numpy_model_matches_breadth_first_search(connectivity, through_empty):
    """Random volumes of 4^3 .. 16^3 around the percolation thresholds (and their complements for the EMPTY flood), random
    seeds in and outside M: the frontier model, the plain whole-array iteration and a breadth-first search agree."""
    rng = np.random.default_rng(42 + connectivity + int(through_empty))
    densities = (0.2, 0.3, 0.4) if connectivity == 6 else (0.05, 0.1, 0.15)
    partial = 0
    for S in (4, 8, 11, 16):
        for density in densities:
            for n_seeds in (0, 1, 5):
                solid = rng.random((S, S, S)) < density
                medium = (~solid if through_empty else solid).astype(np.uint8)     # M has the density either way
                seeds = np.zeros((S, S, S), np.uint8)
                seeds[tuple(rng.integers(0, S, (3, n_seeds)))] = 1                   # anywhere: most of them outside M
                inside = np.argwhere(solid)
                seeds[tuple(inside[rng.integers(0, len(inside), n_seeds)].T)] = 1      # and as many inside it
                want = bfs(solid, seeds, connectivity)
                assert np.array_equal(flood_model.flood(medium, seeds, connectivity, through_empty), want), (S, density, n_seeds)
                assert np.array_equal(flood_model.flood_plain(medium, seeds, connectivity, through_empty), want), (S, density, n_seeds)
                partial += 0 < want.sum() < solid.sum()
    assert partial >= 8                       # most cases reach some of M and not all of it


def test_serpentine_is_one_long_path():
    """The constructed worst case: a path whose flood from its first voxel takes as many steps as it has voxels -- under
    26-connectivity one step fewer per right-angle turn, two turns per join of two lines, and no other shortcut."""
    for S, pitch in ((32, 4), (32, 16), (128, 16)):
        vol, start = flood_model.serpentine(S, pitch)
        n = int(vol.sum())
        assert vol[start] and n > S * (S // pitch) ** 2
        deg6 = flood_model.dilate(vol.astype(bool), 6).sum()                  # cheap shape check before the floods
        assert deg6 > n
        if S > 32:
            continue
        seeds = np.zeros_like(vol)
        seeds[start] = 1
        for connectivity in (6, 26):
            assert np.array_equal(flood_model.flood(vol, seeds, connectivity), vol)
            dist = bfs_depth(vol.astype(bool), start, connectivity)
            turns = 2 * ((S // pitch) ** 2 - 1)
            assert dist == (n - 1 if connectivity == 6 else n - 1 - turns), (S, pitch, connectivity, dist, n)


def bfs_depth(M, start, connectivity):
    S = M.shape[0]
    steps = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    dist = {start: 0}
    queue = deque([start])
    while queue:
        p = queue.popleft()
        for d in steps:
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if min(q) < 0 or max(q) >= S or q in dist or not M[q]:
                continue
            dist[q] = dist[p] + 1
            queue.append(q)
    return max(dist.values())
