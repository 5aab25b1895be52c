"""Flood fill by connectivity on the GPU (vrc_volume_flood, VoxelVolume.flood / keepConnected).  The expected region is
the numpy model of tests/flood_model.py (held against a breadth-first search in tests/test_volume_flood_host.py) on the
same occupancy and seeds; every comparison is exact: the downloaded region equals the model's array and stats.reached
its sum.  No test takes converged == 0 for an answer: a capped call is checked as a partial result and continued."""
import ctypes as C

import numpy as np
import pytest

import flood_model
import raygen
from volume_support import Stream, committed, expected_nodes, same, volume_of

pytestmark = pytest.mark.gpu


def fill_boxes(vol, boxes):
    for x0, y0, z0, x1, y1, z1 in boxes:
        vol[x0:x1, y0:y1, z0:z1] = 1


def flood_and_check(region, medium, medium_np, seeds_np, connectivity, through_empty, what):
    """one uncapped flood against the model; returns (the model's region, the stats)"""
    want = flood_model.flood(medium_np, seeds_np, connectivity, through_empty)
    st = region.flood(medium, connectivity, through_empty)
    assert st.converged == 1, what
    assert np.array_equal(region.download(), want), what
    assert st.reached == int(want.sum(dtype=np.int64)) == region.solidCount(), what
    return want, st


# ---- random volumes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("through_empty", [False, True])
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("depth", [2, 3, 5, 6, 7])
def test_random_volumes(built, depth, connectivity, through_empty):
    """M of random density around the percolation threshold (faces: 0.2 .. 0.4, all 26: 0.05 .. 0.15): many ragged
    components that cross word and tile borders.  Seeds: random voxels, half of them in M, and random small boxes."""
    S = 1 << depth
    rng = np.random.default_rng(7000 + 100 * depth + connectivity + int(through_empty))
    densities = (0.2, 0.31, 0.4) if connectivity == 6 else (0.05, 0.1, 0.15)
    reached_some = 0
    for density in densities:
        in_m = rng.random((S, S, S)) < density
        in_m[tuple(rng.integers(0, S, 3))] = True                # 4^3 at 5 %: never an empty M
        medium_np = (~in_m if through_empty else in_m).astype(np.uint8)
        medium = volume_of(medium_np, depth)
        n = max(2, S // 4)
        inside = np.argwhere(in_m)
        voxels = np.concatenate([rng.integers(0, S, (n, 3)), inside[rng.integers(0, len(inside), n)]])
        lo = rng.integers(0, S, (n, 3))
        boxes = np.concatenate([lo, np.minimum(S, lo + rng.integers(1, 4, (n, 3)))], axis=1)
        seeds_np = np.zeros((S, S, S), np.uint8)
        seeds_np[tuple(voxels.T)] = 1
        fill_boxes(seeds_np, boxes)
        region = volume_of(np.zeros((1, 1, 1)), depth)
        region.setVoxels(voxels)
        region.fillBoxes(boxes)
        want, st = flood_and_check(region, medium, medium_np, seeds_np, connectivity, through_empty, (depth, connectivity, through_empty, density))
        print(f"depth {depth} conn {connectivity} empty {through_empty} density {density}: reached {st.reached} of {int(in_m.sum())} in {st.sweeps} sweeps")
        reached_some += 0 < want.sum() < in_m.sum()
        region.close()
        medium.close()
    assert reached_some >= 1 or depth < 5     # the cases are not all "nothing" or "everything"


# ---- constructed cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [32, 8, 33, 64])
@pytest.mark.parametrize("contact", ["edge", "corner"])
def test_bodies_touching_by_an_edge_or_a_corner(built, p, contact):
    """Two 3^3 bodies that meet only along an edge / at a corner lying at p on every axis: on a tile border (32, 64), a word
    border (8) and inside a brick (33).  Separate under 6, joined under 26."""
    depth, S = 7, 128
    medium_np = np.zeros((S, S, S), np.uint8)
    medium_np[p - 3:p, p - 3:p, p - 3:p] = 1
    if contact == "edge":
        for axis in range(3):                                   # one partner per edge direction, each meeting A along one edge
            b = [slice(p, p + 3)] * 3
            b[axis] = slice(p - 3, p)
            other = medium_np.copy()
            other[tuple(b)] = 1
            _check_contact(other, depth, p, 27, 54)
        return
    medium_np[p:p + 3, p:p + 3, p:p + 3] = 1
    _check_contact(medium_np, depth, p, 27, 54)


def _check_contact(medium_np, depth, p, alone, joined):
    medium = volume_of(medium_np, depth)
    seeds_np = np.zeros_like(medium_np)
    seeds_np[p - 2, p - 2, p - 2] = 1
    for connectivity, count in ((6, alone), (26, joined)):
        region = volume_of(seeds_np, depth)
        want, st = flood_and_check(region, medium, medium_np, seeds_np, connectivity, False, (p, connectivity))
        assert st.reached == count
        region.close()
    medium.close()


@pytest.mark.parametrize("depth,pitch", [(5, 4), (7, 16)])
def test_serpentine(built, depth, pitch):
    """A one-voxel path through every tile of the volume, flooded from its first voxel: with the library's bound, and
    capped at 3 sweeps per call until converged.  Both end at the model's result; a capped call's region is a superset
    of the seed and a subset of the answer, grows from call to call, and the sequence needs more than one call."""
    S = 1 << depth
    medium_np, start = flood_model.serpentine(S, pitch)
    medium = volume_of(medium_np, depth)
    seeds_np = np.zeros_like(medium_np)
    seeds_np[start] = 1
    for connectivity in (6, 26):
        region = volume_of(seeds_np, depth)
        want, st = flood_and_check(region, medium, medium_np, seeds_np, connectivity, False, (depth, connectivity))
        assert np.array_equal(want, medium_np)
        print(f"serpentine {S}^3, {int(want.sum())} voxels, conn {connectivity}: {st.sweeps} sweeps with the library's bound")
        region.close()

        region = volume_of(seeds_np, depth)
        calls, reached, total = 0, 1, int(want.sum())
        while True:
            st = region.flood(medium, connectivity, False, 3)
            calls += 1
            assert st.sweeps <= 3
            assert st.reached >= reached and (st.converged or st.reached > reached), "a capped call made no progress"
            reached = st.reached
            if calls <= 2 or st.converged:
                got = region.download()
                assert got[start] == 1 and not np.any(got > want), calls           # seed kept, nothing outside the answer
                assert int(got.sum()) == st.reached
            if st.converged:
                break
            assert calls <= total, "more capped calls than the path has voxels"
        assert calls > 1
        assert np.array_equal(got, want) and st.reached == total
        print(f"serpentine {S}^3 conn {connectivity}: {calls} calls of at most 3 sweeps")
        region.close()
    medium.close()


def test_sealed_hollow_box(built):
    """EMPTY floods: from outside a sealed shell the cavity stays dry; from inside exactly the cavity fills; a room closed
    by a wall on one side and the volume's faces on the others fills up to the faces and no further."""
    depth, S = 6, 64
    medium_np = np.zeros((S, S, S), np.uint8)
    medium_np[10:40, 9:41, 7:42] = 1
    medium_np[11:39, 10:40, 8:41] = 0                           # the cavity straddles the tile border at 32
    cavity = np.zeros_like(medium_np)
    cavity[11:39, 10:40, 8:41] = 1
    medium = volume_of(medium_np, depth)
    for connectivity in (6, 26):
        for seed, expect in (((0, 0, 0), (1 - medium_np) & (1 - cavity)), ((20, 33, 12), cavity)):
            seeds_np = np.zeros_like(medium_np)
            seeds_np[seed] = 1
            region = volume_of(seeds_np, depth)
            want, _ = flood_and_check(region, medium, medium_np, seeds_np, connectivity, True, (connectivity, seed))
            assert np.array_equal(want, expect)
            region.close()
    medium.close()
    medium_np[:] = 0
    medium_np[20, :, :] = 1                                     # a wall from face to face
    medium = volume_of(medium_np, depth)
    seeds_np = np.zeros_like(medium_np)
    seeds_np[5, 63, 0] = 1
    region = volume_of(seeds_np, depth)
    want, st = flood_and_check(region, medium, medium_np, seeds_np, 26, True, "room")
    assert st.reached == 20 * S * S and not want[21:].any()
    region.close()
    medium.close()


@pytest.mark.parametrize("depth", [2, 3, 4, 6])
def test_solid_up_to_the_faces_does_not_wrap(built, depth):
    """A medium solid up to every face, cut in two by an empty slab: the flood from one half fills it to the faces and
    does not come round to the other half."""
    S = 1 << depth
    medium_np = np.ones((S, S, S), np.uint8)
    medium_np[:, S // 2, :] = 0
    medium = volume_of(medium_np, depth)
    for connectivity in (6, 26):
        for seed in ((0, 0, 0), (S - 1, S - 1, S - 1), (S - 1, 0, S - 1)):
            seeds_np = np.zeros_like(medium_np)
            seeds_np[seed] = 1
            region = volume_of(seeds_np, depth)
            want, st = flood_and_check(region, medium, medium_np, seeds_np, connectivity, False, (depth, connectivity, seed))
            low = seed[1] < S // 2
            assert st.reached == S * S * (S // 2 if low else S // 2 - 1)
            assert not (want[:, S // 2:, :] if low else want[:, :S // 2 + 1, :]).any()
            region.close()
    medium.close()


# ---- seeds ------------------------------------------------------------------------------------------------------

def test_seeds(built):
    depth, S = 6, 64
    rng = np.random.default_rng(61)
    medium_np = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
    medium = volume_of(medium_np, depth)
    # seeds not in M are dropped: a region of seeds that all lie outside M ends empty
    outside = np.argwhere(medium_np == 0)[::500]
    seeds_np = np.zeros_like(medium_np)
    seeds_np[tuple(outside.T)] = 1
    region = volume_of(seeds_np, depth)
    want, st = flood_and_check(region, medium, medium_np, seeds_np, 6, False, "seeds outside M")
    assert st.reached == 0 and len(outside) > 100
    # ... and next to seeds inside M they leave no trace
    seeds_np[tuple(np.argwhere(medium_np)[::900].T)] = 1
    region.setVoxels(np.argwhere(seeds_np))
    want, st = flood_and_check(region, medium, medium_np, seeds_np, 6, False, "mixed seeds")
    assert st.reached > 0 and not np.any(want & (1 - medium_np))
    # a region that is already the answer is left unchanged, and says so at once
    again = region.flood(medium, 6)
    assert again.converged == 1 and again.reached == st.reached and again.sweeps <= 4
    assert np.array_equal(region.download(), want)
    region.close()
    # an empty seed set
    for through_empty in (False, True):
        region = volume_of(np.zeros((1, 1, 1)), depth)
        st = region.flood(medium, 26, through_empty)
        assert st.converged == 1 and st.reached == 0 and st.sweeps <= 4
        assert not region.download().any()
        region.close()
    medium.close()


# ---- refusals on live volumes -----------------------------------------------------------------------------------

def test_volumes_of_different_depths_are_refused(built):
    """A depth-5 region against a depth-6 medium and the other way round: VRC_ERR_INVALID with the function's name, both
    volumes as they were, the stats untouched.  (The check is what keeps the kernels from indexing one volume with the
    other's extents.)  Volumes on different devices are refused by the same chain of checks; that needs two GPUs and is
    not exercised here."""
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    rng = np.random.default_rng(56)
    small_np = (rng.random((32, 32, 32)) < 0.3).astype(np.uint8)
    large_np = (rng.random((64, 64, 64)) < 0.3).astype(np.uint8)
    small, large = volume_of(small_np, 5), volume_of(large_np, 6)
    for region, medium in ((small, large), (large, small)):
        for connectivity in (6, 26):
            for through in (0, 1):
                st = vrc.capi.FloodStats(reached=7, sweeps=7, converged=7)
                assert L.vrc_volume_flood(region._h, medium._h, connectivity, through, 0, C.byref(st)) == -1
                assert L.vrc_last_error().startswith(b"vrc_volume_flood"), L.vrc_last_error()
                assert (st.reached, st.sweeps, st.converged) == (7, 7, 7)
                assert L.vrc_volume_flood(region._h, medium._h, connectivity, through, 3, None) == -1
        with pytest.raises(vrc.VrcError, match="vrc_volume_flood"):
            region.flood(medium)
    assert np.array_equal(small.download(), small_np) and np.array_equal(large.download(), large_np)
    assert L.vrc_volume_flood(small._h, small._h, 6, 0, 0, None) == -1          # the same live volume twice
    assert L.vrc_last_error().startswith(b"vrc_volume_flood")
    assert np.array_equal(small.download(), small_np)
    small.close()
    large.close()


# ---- ordering ---------------------------------------------------------------------------------------------------

def test_flood_behind_device_edits_and_commit_after(built):
    """Asynchronous device-memory edits of region and of medium on a caller's stream immediately before the flood are
    seen by it; a commit of region right after the flood gives the host builder's array for the model's occupancy."""
    import torch
    depth, S = 7, 128
    rng = np.random.default_rng(77)
    medium_np = (rng.random((S, S, S)) < 0.27).astype(np.uint8)
    medium = volume_of(medium_np, depth)
    region = volume_of(np.zeros((1, 1, 1)), depth)
    # the edits: a bridge of boxes and many voxels added to the medium, seeds put into the region -- none of it on the host path
    boxes = np.array([[0, 60, 60, S, 62, 62], [60, 0, 60, 62, S, 62], [60, 60, 0, 62, 62, S]], np.uint32)
    extra = rng.integers(0, S, (200000, 3)).astype(np.uint32)
    seeds = np.array([[0, 60, 60], [5, 5, 5], [127, 127, 127]], np.uint32)
    seed_boxes = np.array([[30, 30, 30, 34, 34, 34]], np.uint32)
    t_boxes, t_extra = torch.from_numpy(boxes.view(np.int32)).cuda(), torch.from_numpy(extra.view(np.int32)).cuda()
    t_seeds, t_seed_boxes = torch.from_numpy(seeds.view(np.int32)).cuda(), torch.from_numpy(seed_boxes.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        medium.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
        medium.fillBoxesDevice(len(boxes), t_boxes.data_ptr(), True, stream)
        region.setVoxelsDevice(len(seeds), t_seeds.data_ptr(), True, stream)
        region.fillBoxesDevice(len(seed_boxes), t_seed_boxes.data_ptr(), True, stream)
        st = region.flood(medium, 6)                            # nothing between the edits and the flood
        nodes = committed(region)                               # ... nor between the flood and the commit
    medium_np[tuple(extra.astype(np.int64).T)] = 1
    fill_boxes(medium_np, boxes.astype(np.int64))
    seeds_np = np.zeros_like(medium_np)
    seeds_np[tuple(seeds.astype(np.int64).T)] = 1
    fill_boxes(seeds_np, seed_boxes.astype(np.int64))
    want = flood_model.flood(medium_np, seeds_np, 6)
    assert np.array_equal(medium.download(), medium_np)
    assert st.converged == 1 and st.reached == int(want.sum()) and st.reached > 3 * S
    assert np.array_equal(region.download(), want)
    assert same(nodes, expected_nodes(want, depth))
    region.close()
    medium.close()


# ---- the user's story at full size ------------------------------------------------------------------------------

def test_dig_then_keep_connected_at_512(built):
    """The 512^3 FastNoise terrain as a volume; rays cast on the device, a sphere dug at every hit on the same stream,
    keepConnected anchored on the slab the terrain's columns stand on (y = S/2 + 1, main.cpp:65-74).  supported | debris is
    the dug volume, they do not overlap, supported is the model's flood of the downloaded dug volume; the committed scene
    is the host builder's array for it and renders the frame a scene built from the model's occupancy renders.  A 3^3
    block is set in the empty half of the volume (the columns start at y = S/2 + 1; the block ends three voxels short of
    it) before keepConnected, so that the debris is never empty whatever the digs detach."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S, radius = 9, 512, 9
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    org, d = raygen.camera_rays(depth, 96, 54, -0.5)
    n = len(org)
    t_org, t_dir = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    t_hits = torch.zeros(n * 12, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        scene.castRaysDevice(n, t_org.data_ptr(), t_dir.data_ptr(), t_hits.data_ptr(), stream=stream)
        volume.fillSpheresAtHitsDevice(n, t_hits.data_ptr(), radius, False, stream)
        floating = np.array([[100, S // 2 - 5, 100, 103, S // 2 - 2, 103]], np.uint32)
        volume.fillBoxes(floating)
        dug = volume.download()
        anchors = np.array([[0, S // 2 + 1, 0, S, S // 2 + 2, S]], np.uint32)
        debris = volume.keepConnected(anchors)
    before = int(dug.sum(dtype=np.int64))
    supported_np, debris_np = volume.download(), debris.download()
    seeds_np = np.zeros_like(dug)
    fill_boxes(seeds_np, anchors.astype(np.int64))
    want = flood_model.flood(dug, seeds_np, 6)
    n_supported, n_debris = int(supported_np.sum(dtype=np.int64)), int(debris_np.sum(dtype=np.int64))
    print(f"512^3 story: {n} rays, radius {radius}: {before} solid after the dig, {n_supported} supported, {n_debris} debris")
    assert np.array_equal(supported_np | debris_np, dug)
    assert not np.any(supported_np & debris_np)
    assert np.array_equal(supported_np, want)
    assert n_supported + n_debris == before == volume.solidCount() + debris.solidCount()
    assert n_supported > 0 and n_debris >= 27
    assert debris_np[100:103, S // 2 - 5:S // 2 - 2, 100:103].all() and not supported_np[100:103, S // 2 - 5:S // 2 - 2, 100:103].any()
    after = volume.commit()
    assert same(after.downloadNodes(), vrc.build_volume_lsvo(want, depth))
    # the committed scene is a usable one: a small frame through setScene equals the frame of the model's scene
    cam = vrc.reference_camera(depth, pitch=-0.5)
    images = []
    for via_set_scene in (True, False):
        model_scene = vrc.LSVO.fromVolume(want, depth)
        rc = vrc.RayCaster(scene if via_set_scene else model_scene, (64, 36))
        rc.setLightPosition(vrc.reference_light(depth))
        if via_set_scene:
            rc.setScene(after)
        rc.renderFrame(cam)
        images.append(rc.readImage())
        rc.close()
        model_scene.close()
    assert np.array_equal(images[0], images[1])
    assert len(np.unique(images[0].reshape(-1, 4), axis=0)) > 1  # terrain and sky, not one flat colour
    for v in (after, debris, volume, scene):
        v.close()


# ---- no growth --------------------------------------------------------------------------------------------------

def test_floods_do_not_grow(built):
    """Twenty floods on one pair of volumes leave the device's free memory where the second left it."""
    import torch
    depth, S = 7, 128
    rng = np.random.default_rng(5)
    medium_np = (rng.random((S, S, S)) < 0.32).astype(np.uint8)
    medium = volume_of(medium_np, depth)
    seeds = np.concatenate([np.argwhere(medium_np)[::5000], np.argwhere(medium_np == 0)[::5000]])   # some in M whichever M is
    region = volume_of(np.zeros((1, 1, 1)), depth)
    free = []
    for i in range(20):
        region.fillBoxes(np.array([[0, 0, 0, S, S, S]], np.uint32), False)
        region.setVoxels(seeds)
        st = region.flood(medium, 6 if i % 2 else 26, bool(i % 3 == 0))
        assert st.converged == 1 and st.reached > 0
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[1] == free[19], free
    region.close()
    medium.close()
