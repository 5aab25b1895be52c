"""The editable voxel volume on the GPU (vrc_volume_*, vrc_renderer_set_scene): every committed scene against the
array the oracle's SVO::setCell + compileSVO (small depths) or the host builder (depth 8-9, itself held to the oracle
by tests/test_builder.py) produces for the numpy-tracked voxel set -- bit for bit -- and the frames rendered on them."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from volume_support import committed as committed_nodes, expected_nodes, same, terrain_volume

pytestmark = pytest.mark.gpu
committed = functools.partial(committed_nodes, timed=True)      # every commit of this file must also report its build time


# ---- 1. round trip -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [4, 6, 8, 9])
def test_round_trip_terrain(built, heights, depth):
    import cpuvoxelraycaster_amd as vrc
    svo = vrc.LSVO.fromTerrain(heights, depth)
    original = svo.downloadNodes()
    assert same(original, vrc.build_terrain_lsvo(heights, depth))
    volume = vrc.VoxelVolume.fromScene(svo)
    svo.close()                                      # the volume does not depend on the scene it came from
    dense = terrain_volume(heights, depth)
    assert np.array_equal(volume.download(), dense)
    assert volume.solidCount() == int(dense.sum(dtype=np.int64))
    assert same(committed(volume), original)
    assert same(committed(volume), original)         # and again: a commit leaves the volume as it was


def test_round_trip_fastnoise_512(built, heights):
    import cpuvoxelraycaster_amd as vrc
    svo = vrc.LSVO.fromFastNoiseTerrain(9)
    original = svo.downloadNodes()
    assert len(original) == 10528393
    volume = vrc.VoxelVolume.fromScene(svo)
    assert volume.solidCount() == 8583552
    assert np.array_equal(volume.download(), terrain_volume(heights, 9))
    assert same(committed(volume), original)


# ---- 2. random edits -----------------------------------------------------------------------------------------

def edge_voxels(S):
    """every corner, and one voxel inside every face"""
    c = [(x, y, z) for x in (0, S - 1) for y in (0, S - 1) for z in (0, S - 1)]
    m = S // 2
    f = [(0, m, m - 1), (S - 1, m, m - 1), (m, 0, m - 1), (m, S - 1, m - 1), (m, m - 1, 0), (m, m - 1, S - 1)]
    return np.array(c + f, np.int64)


@pytest.mark.parametrize("depth", [2, 3, 5])
@pytest.mark.parametrize("density", [0.0, 0.3, 1.0])
def test_random_edit_batches(built, depth, density):
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    rng = np.random.default_rng(depth * 100 + int(density * 10))
    vol = (rng.random((S, S, S)) < density).astype(np.uint8)
    if density == 0.0:
        volume = vrc.VoxelVolume(depth)
    else:
        start = vrc.LSVO.fromVolume(vol, depth)
        volume = vrc.VoxelVolume.fromScene(start)
        start.close()
    assert np.array_equal(volume.download(), vol)
    outside = np.array([(S, 0, 0), (0, S, 0), (0, 0, S), (S, S, S), (0xffffffff, 1, 1), (1, 0x80000000, 1), (1, 1, 12345678)], np.int64)
    for batch in range(3):
        for solid in ((True, False) if batch != 1 else (False, True)):
            k = int(rng.integers(1, S * S * S // 2 + 2))
            xyz = rng.integers(0, S, (k, 3))
            xyz = np.concatenate([xyz, xyz[: k // 2 + 1], outside, edge_voxels(S)[rng.random(14) < 0.7]])   # duplicates, out-of-volume, faces / corners
            rng.shuffle(xyz)
            volume.setVoxels(xyz.astype(np.uint32), solid)
            inside = xyz[np.all(xyz < S, axis=1)]
            vol[inside[:, 0], inside[:, 1], inside[:, 2]] = 1 if solid else 0
        assert same(committed(volume), expected_nodes(vol, depth)), (depth, density, batch)
        assert volume.solidCount() == int(vol.sum())
    assert np.array_equal(volume.download(), vol)
    everything = np.argwhere(np.ones((S, S, S), bool)).astype(np.uint32)
    volume.setVoxels(everything, False)              # emptied completely: compileSVO's lone root
    empty = committed(volume)
    assert len(empty) == 1 and empty[0]["child_offset"] == 1 and empty[0]["child_mask"] == 0 and volume.solidCount() == 0
    assert same(empty, O.compile_voxels(depth, []))
    volume.setVoxels(np.concatenate([everything, everything[::3]]), True)   # filled completely
    assert same(committed(volume), O.compile_voxels(depth, everything)) and volume.solidCount() == S ** 3
    volume.setVoxels(edge_voxels(S).astype(np.uint32), False)
    full = np.ones((S, S, S), np.uint8)
    e = edge_voxels(S)
    full[e[:, 0], e[:, 1], e[:, 2]] = 0
    assert same(committed(volume), expected_nodes(full, depth))


# ---- 3. boxes ------------------------------------------------------------------------------------------------

def box_cases(S):
    h = S // 2
    return [
        (True, [(0, 0, 0, h, h, h)]),                                     # brick- and word-aligned
        (True, [(h + 1, 3, 5, S - 1, h - 1, S - 3)]),                      # unaligned by one voxel on each side
        (False, [(2, 2, 2, h - 1, h - 2, h - 3)]),                         # carve, unaligned
        (True, [(3, 0, 0, 4, S, S), (0, 5, 0, S, 6, S), (0, 0, 7, S, S, 8)]),   # one voxel thick, each axis
        (True, [(4, 4, 4, 4, 9, 9), (9, 9, 9, 3, 3, 3), (S, 0, 0, S + 4, 4, 4)]),   # empty, inverted, outside
        (False, [(h - 3, h - 3, h - 3, S + 100, 0xffffffff, S)]),          # clipped by the volume
        (True, [(1, 1, 1, h, h, h), (h - 4, h - 4, h - 4, h + 5, h + 5, h + 5), (h - 4, 1, h - 4, h + 5, h, h + 5)]),   # overlapping
        (False, [(0, 0, 0, S, S, 1), (0, 0, S - 1, S, S, S), (0, 0, 1, S, S, 3), (5, 6, 0, 6, 7, S)]),
        (True, [(0, 0, 0, S, S, S)]),                                      # the whole volume
        (False, [(1, 1, 1, S - 1, S - 1, S - 1)]),                         # a shell is left
    ]


@pytest.mark.parametrize("depth", [5, 8])
def test_fill_boxes(built, depth):
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    rng = np.random.default_rng(depth)
    vol = (rng.random((S, S, S)) < 0.05).astype(np.uint8)
    start = vrc.LSVO.fromVolume(vol, depth)
    volume = vrc.VoxelVolume.fromScene(start)
    start.close()
    for i, (solid, boxes) in enumerate(box_cases(S)):
        volume.fillBoxes(np.array(boxes, np.uint64).astype(np.uint32), solid)
        for (x0, y0, z0, x1, y1, z1) in boxes:
            if x0 < x1 and y0 < y1 and z0 < z1:
                vol[x0:min(x1, S), y0:min(y1, S), z0:min(z1, S)] = 1 if solid else 0
        assert np.array_equal(volume.download(), vol), (depth, i)
        assert volume.solidCount() == int(vol.sum(dtype=np.int64))
        if depth == 5 or i in (1, 6, 9):
            assert same(committed(volume), expected_nodes(vol, depth)), (depth, i)
    many = rng.integers(0, S, (300, 6))                                    # many small random boxes in one call
    many[:, 3:] = many[:, :3] + rng.integers(0, 9, (300, 3))
    volume.fillBoxes(many.astype(np.uint32), True)
    for (x0, y0, z0, x1, y1, z1) in many:
        vol[x0:min(x1, S), y0:min(y1, S), z0:min(z1, S)] = 1
    assert np.array_equal(volume.download(), vol)
    assert same(committed(volume), expected_nodes(vol, depth))


# ---- 4. host and device memory forms ---------------------------------------------------------------------------

def test_host_and_device_forms_agree(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth = 6
    S = 1 << depth
    rng = np.random.default_rng(4)
    sets = rng.integers(0, S + 2, (5000, 3)).astype(np.uint32)
    clears = rng.integers(0, S, (3000, 3)).astype(np.uint32)
    lo = rng.integers(0, S, (40, 3))
    boxes = np.concatenate([lo, lo + rng.integers(0, 12, (40, 3))], axis=1).astype(np.uint32)
    carve = np.array([[10, 11, 12, 30, 29, 31]], np.uint32)
    host, dev = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
    host.setVoxels(sets, True)
    host.fillBoxes(boxes, True)
    host.setVoxels(clears, False)
    host.fillBoxes(carve, False)
    L = vrc.capi.load()
    stream = C.c_void_p()
    vrc.capi.check(L.vrc_stream_create(0, C.byref(stream)))
    try:
        t = [torch.from_numpy(a.view(np.int32).copy()).cuda() for a in (sets, boxes, clears, carve)]
        torch.cuda.synchronize()
        dev.setVoxelsDevice(len(sets), t[0].data_ptr(), True, stream)
        dev.fillBoxesDevice(len(boxes), t[1].data_ptr(), True, stream)
        dev.setVoxelsDevice(len(clears), t[2].data_ptr(), False, stream)
        dev.fillBoxesDevice(len(carve), t[3].data_ptr(), False, stream)
        got = committed(dev)                          # a commit waits for the edits issued so far, whatever their stream
        vrc.capi.check(L.vrc_stream_synchronize(0, stream))
    finally:
        L.vrc_stream_destroy(0, stream)
    vol = np.zeros((S, S, S), np.uint8)
    inside = sets[np.all(sets < S, axis=1)]
    vol[inside[:, 0], inside[:, 1], inside[:, 2]] = 1
    for (x0, y0, z0, x1, y1, z1) in boxes:
        vol[x0:min(x1, S), y0:min(y1, S), z0:min(z1, S)] = 1
    vol[clears[:, 0], clears[:, 1], clears[:, 2]] = 0
    vol[10:30, 11:29, 12:31] = 0
    assert np.array_equal(host.download(), vol) and np.array_equal(dev.download(), vol)
    assert same(got, committed(host)) and same(got, expected_nodes(vol, depth))


# ---- 5. dig and build at the hit -------------------------------------------------------------------------------

def autofocus_ray(depth, cam):
    S = np.float32(1 << depth)
    org = (np.array(tuple(cam.position), np.float32) / S + np.float32(1.0)).astype(np.float32)
    rot = np.array(tuple(cam.rot), np.float32)
    return org, np.array([rot[2], rot[5], rot[8]], np.float32)        # Camera::getClosestPoint, camera_controller.hpp:56-60


def test_dig_and_build_at_the_hit(built, heights):
    import cpuvoxelraycaster_amd as vrc
    depth = 8
    vol = terrain_volume(heights, depth)
    scene = vrc.LSVO.fromTerrain(heights, depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    org, d = autofocus_ray(depth, vrc.reference_camera(depth, pitch=-0.5))
    first = scene.castRay(org, d)
    voxel, neighbour = vrc.hit_to_voxel(depth, first)
    assert vol[voxel] == 1 and neighbour is not None and vol[neighbour] == 0
    # dig: the voxel under the crosshair goes, the ray goes on to whatever lies behind it
    volume.setVoxels([voxel], False)
    vol[voxel] = 0
    dug = volume.commit()
    want_nodes = expected_nodes(vol, depth)
    assert same(dug.downloadNodes(), want_nodes)
    second = dug.castRay(org, d)
    want = O.cast_rays(want_nodes, depth, org[None], d[None])[0]
    assert second.tobytes() == want.tobytes()
    assert (second["hit"] & 0xff) == 1 and second["distance"] > first["distance"]
    assert vrc.hit_to_voxel(depth, second)[0] != voxel
    # build: the empty cell the first ray came through becomes solid, and is what the ray now hits
    volume.setVoxels([neighbour], True)
    vol[neighbour] = 1
    raised = volume.commit()
    want_nodes = expected_nodes(vol, depth)
    assert same(raised.downloadNodes(), want_nodes)
    third = raised.castRay(org, d)
    assert third.tobytes() == O.cast_rays(want_nodes, depth, org[None], d[None])[0].tobytes()
    assert vrc.hit_to_voxel(depth, third)[0] == neighbour and third["distance"] < first["distance"]
    # the scenes committed earlier are what they were
    assert scene.castRay(org, d).tobytes() == first.tobytes() and dug.castRay(org, d).tobytes() == second.tobytes()


# ---- 6. setScene -----------------------------------------------------------------------------------------------

def oracle_frame(nodes, depth, textures, cam, light, W, H, spp):
    top, side = textures
    ocam = O.make_camera(tuple(cam.position), tuple(cam.rot), cam.fov, cam.aperture, cam.focal_length)
    acc, rays, steps = None, 0, 0
    for s in range(spp):
        p = O.make_params(W, H, light, use_gi=1, use_samples=1, shadow_samples=1, frame_index=s)
        _, acc, _, st = O.render_frame(nodes, depth, top, side, ocam, p, accum=acc, threads=8)
        rays, steps = rays + st.rays, steps + st.sum_complexity
    return acc, (rays, steps, W * H * spp)


def stats_tuple(st):
    return (st.rays, st.sum_complexity, st.pixels)     # the counters the oracle keeps as well


def cleared_box_in_view(depth, scene, cam):
    """a 16^3 box around the voxel under the crosshair"""
    import cpuvoxelraycaster_amd as vrc
    org, d = autofocus_ray(depth, cam)
    voxel, _ = vrc.hit_to_voxel(depth, scene.castRay(org, d))
    lo = [max(0, c - 8) for c in voxel]
    return lo + [c + 16 for c in lo]


def test_set_scene_keeps_the_renderer(built, heights, textures):
    import cpuvoxelraycaster_amd as vrc
    depth, W, H, spp = 8, 320, 180, 2
    vol = terrain_volume(heights, depth)
    a = vrc.LSVO.fromTerrain(heights, depth, textures=textures)
    cam, light = vrc.reference_camera(depth, pitch=-0.5), vrc.reference_light(depth)
    box = cleared_box_in_view(depth, a, cam)
    volume = vrc.VoxelVolume.fromScene(a)
    volume.fillBoxes([box], False)
    vol[box[0]:box[3], box[1]:box[4], box[2]:box[5]] = 0
    b = volume.commit()                              # carries A's albedo tables
    nodes_b = b.downloadNodes()
    assert same(nodes_b, expected_nodes(vol, depth))

    rc = vrc.RayCaster(a, (W, H))
    rc.setLightPosition(light)
    rc.use_gi = rc.use_samples = True
    rc.shadow_samples = 1
    rc.renderFrame(cam, spp=spp)
    acc_a = rc.readAccum()
    want_a, stats_a = oracle_frame(a.downloadNodes(), depth, textures, cam, light, W, H, spp)
    assert np.array_equal(acc_a, want_a) and stats_tuple(rc.stats()) == stats_a
    rc.setScene(b)
    assert np.array_equal(rc.readAccum(), acc_a) and stats_tuple(rc.stats()) == stats_a     # kept across the rebind
    rc.resetSamples()
    rc.stats(reset=True)
    rc.frame_index = 0
    rc.renderFrame(cam, spp=spp)
    want_b, stats_b = oracle_frame(nodes_b, depth, textures, cam, light, W, H, spp)
    assert np.array_equal(rc.readAccum(), want_b) and stats_tuple(rc.stats()) == stats_b
    assert not np.array_equal(want_a, want_b)
    # refusals: another depth
    other = vrc.LSVO.fromTerrain(heights, 7)
    with pytest.raises(vrc.VrcError):
        rc.setScene(other)


def test_commit_does_not_disturb_a_frame_in_flight(built, heights, textures):
    """A frame enqueued on scene A on one stream; a commit and a frame on the new scene B on another: both frames
    match their oracles."""
    import cpuvoxelraycaster_amd as vrc
    depth, W, H, spp = 8, 320, 180, 2
    vol = terrain_volume(heights, depth)
    a = vrc.LSVO.fromTerrain(heights, depth, textures=textures)
    nodes_a = a.downloadNodes()
    cam, light = vrc.reference_camera(depth, pitch=-0.5), vrc.reference_light(depth)
    box = cleared_box_in_view(depth, a, cam)
    volume = vrc.VoxelVolume.fromScene(a)
    committed(volume)                                # the volume's grids exist: the commit below only launches kernels

    def renderer(svo):
        rc = vrc.RayCaster(svo, (W, H))
        rc.setLightPosition(light)
        rc.use_gi = rc.use_samples = True
        rc.shadow_samples = 1
        return rc

    rc_a, rc_b = renderer(a), renderer(a)
    L = vrc.capi.load()
    s1, s2 = C.c_void_p(), C.c_void_p()
    vrc.capi.check(L.vrc_stream_create(0, C.byref(s1)))
    vrc.capi.check(L.vrc_stream_create(0, C.byref(s2)))
    try:
        rc_a.renderFrame(cam, spp=spp, stream=s1)    # in flight on A ...
        volume.fillBoxes([box], False)
        b = volume.commit()                          # ... while B is built
        rc_b.setScene(b)
        rc_b.renderFrame(cam, spp=spp, stream=s2)
        acc_a, acc_b = rc_a.readAccum(stream=s1), rc_b.readAccum(stream=s2)
        st_a, st_b = stats_tuple(rc_a.stats(stream=s1)), stats_tuple(rc_b.stats(stream=s2))
    finally:
        L.vrc_stream_synchronize(0, s1)
        L.vrc_stream_synchronize(0, s2)
        L.vrc_stream_destroy(0, s1)
        L.vrc_stream_destroy(0, s2)
    vol[box[0]:box[3], box[1]:box[4], box[2]:box[5]] = 0
    nodes_b = b.downloadNodes()
    assert same(nodes_b, expected_nodes(vol, depth)) and same(a.downloadNodes(), nodes_a)
    want_a, stats_a = oracle_frame(nodes_a, depth, textures, cam, light, W, H, spp)
    want_b, stats_b = oracle_frame(nodes_b, depth, textures, cam, light, W, H, spp)
    assert np.array_equal(acc_a, want_a) and st_a == stats_a
    assert np.array_equal(acc_b, want_b) and st_b == stats_b


# ---- 7. repeated commits ---------------------------------------------------------------------------------------

def test_repeated_commits_alternate_and_do_not_grow(built, heights):
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth = 8
    S = 1 << depth
    vol = terrain_volume(heights, depth)
    scene = vrc.LSVO.fromTerrain(heights, depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    scene.close()
    box = [S // 2 - 20, S // 2 - 10, S // 2 - 20, S // 2 + 21, S // 2 + 31, S // 2 + 19]
    with_box = vol.copy()
    with_box[box[0]:box[3], box[1]:box[4], box[2]:box[5]] = 1
    back = with_box.copy()                           # the box cleared again: not the terrain (it ate into the hill)
    back[box[0]:box[3], box[1]:box[4], box[2]:box[5]] = 0
    want = [expected_nodes(with_box, depth), expected_nodes(back, depth)]
    assert not same(want[0], want[1])
    used = {}
    for i in range(1, 21):
        volume.fillBoxes([box], i % 2 == 1)
        assert same(committed(volume), want[(i + 1) % 2]), i
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        used[i] = total - free
    print("device memory in use after commit 3, 4, 19, 20:", used[3], used[4], used[19], used[20])
    assert used[19] <= used[3] and used[20] <= used[4]
