"""Solid voxelisation of triangle meshes on the GPU (vrc_volume_xor_mesh, VoxelVolume.xorMesh / voxelizeMesh / stampMesh).
The expected occupancy is the numpy model of tests/voxelize_model.py (held against boxes, a fan and an exact orientation
test in tests/test_volume_voxelize_host.py); every comparison is exact: the downloaded volume equals the model's array.
Shapes are the smallest at which the kernels take another path: 4^3 (two brick rows to a word), 8^3 (one z word per
column), 32^3 (four), 64^3 (more than one workgroup in the scan, a triangle split over several workgroups in the mark).
The scan's other lane counts (2, 16, 32, 64 and two words a lane) and the stride of the mark loop: test_gpu_volume_voxelize_large.py."""

import numpy as np
import pytest

import voxelize_model as M
from volume_support import Stream, same

pytestmark = pytest.mark.gpu
U = M.UNIT


def voxelised(depth, tris, before=None):
    """the downloaded volume after one host-memory xorMesh into `before` (dense) or an empty volume"""
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(depth)
    if before is not None and before.any():
        volume.setVoxels(np.argwhere(before))
    volume.xorMesh(tris)
    got = volume.download()
    volume.close()
    return got


def check(depth, tris, what, before=None):
    S = 1 << depth
    want = M.xor_mesh(S, tris, None if before is None else before.copy())
    got = voxelised(depth, tris, before)
    assert np.array_equal(got, want), (what, int(got.sum()), int(want.sum()), np.argwhere(got != want)[:8].tolist())
    return want


def tetrahedron(S, rng):
    """a closed tetrahedron with a vertex beyond every face of the volume, below z = 0 and above z = S among them"""
    v = np.array([(-0.4, -0.3, -0.5), (1.5, -0.2, 0.3), (0.4, 1.6, -0.1), (0.5, 0.4, 1.7)]) * S + rng.uniform(-0.1, 0.1, (4, 3)) * S
    return M.soup(M.quantise(v), [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)])


def sphere(S, radius, centre, subdivisions=2):
    import cpuvoxelraycaster_amd as vrc
    verts, faces = vrc.icosphere(subdivisions)
    return M.soup(M.quantise(verts, radius, centre), faces)


def box(lo, hi):
    import cpuvoxelraycaster_amd as vrc
    verts, faces = vrc.box_mesh(lo, hi)
    return M.soup(M.quantise(verts), faces)


def sheet(x0, y0, x1, y1, h):
    """an open horizontal rectangle [x0, x1] x [y0, y1] (voxels) at height h (units): two triangles"""
    a, b, c, d = (x0 * U, y0 * U, h), (x1 * U, y0 * U, h), (x1 * U, y1 * U, h), (x0 * U, y1 * U, h)
    return np.array([a + b + c, a + c + d], np.int32)


# ---- closed meshes at every depth with a path of its own -----------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3, 5, 6])
def test_closed_meshes_sticking_out_of_every_face(built, depth):
    S = 1 << depth
    rng = np.random.default_rng(100 + depth)
    want = check(depth, tetrahedron(S, rng), "tetrahedron")
    assert 0 < want.sum() < S ** 3
    # radius 0.7 S around the middle: the ball leaves through all six faces and the volume's corners stay outside it
    want = check(depth, sphere(S, 0.7 * S, (S / 2 + 0.3, S / 2 - 0.2, S / 2 + 0.1)), "icosphere")
    assert want[S // 2, S // 2, 0] and want[S // 2, S // 2, S - 1]
    assert depth == 2 or not (want[0, 0, 0] or want[S - 1, S - 1, S - 1])     # at 4^3 the corner voxels' centres are inside
    for i in range(3):                                                 # wholly random ones, some of them slivers
        v = rng.integers(-S * U // 2, 3 * S * U // 2, (4, 3))
        check(depth, M.soup(v, [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]), ("random tetrahedron", i))


@pytest.mark.parametrize("depth", [2, 3, 5, 6])
def test_integer_box_equals_fill_boxes(built, depth):
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    for lo, hi in (((1, 0, 1), (S - 1, S // 2, S)), ((0, 0, 0), (S, S, S)), ((S // 4, 1, S // 2 - 1), (S // 4 + 1, 3, S // 2 + 1))):
        got = voxelised(depth, box(lo, hi))
        filled = vrc.VoxelVolume(depth)
        filled.fillBoxes([list(lo) + list(hi)])
        assert np.array_equal(got, filled.download()), (lo, hi)
        assert got.sum() == np.prod(np.subtract(hi, lo))
        filled.close()
        check(depth, box(lo, hi), (lo, hi))


def test_half_voxel_box(built):
    want = check(5, box((2.5, 3.5, 1.5), (10.5, 8.5, 29.5)), "half-voxel box")
    assert want.sum() == 8 * 5 * 28


@pytest.mark.parametrize("depth", [2, 3, 5])
def test_fan_and_its_mirrored_copies(built, depth):
    """Four triangles meeting at a column centre, diagonals through column centres, all eight mirrored / transposed copies
    (every edge in every orientation), at heights between voxel centres and exactly through them."""
    import test_volume_voxelize_host as H
    S = 1 << depth
    for mx, my, sw in H.FAN_VARIANTS:
        for h in (5 * U, 5 * U + M.HALF, 5 * U + M.HALF + 1, M.HALF, M.HALF + 1, 40 * U, -U):
            tris = H.fan(h, mx, my, sw)
            want = check(depth, tris, (mx, my, sw, h))
            k = int(np.clip(-((M.HALF - h) // U), 0, S))
            assert want.sum() == min(9, S) ** 2 * k


def test_crossings_at_nibble_word_and_column_borders(built):
    """One-column sheets with k = 1, 8, 9, 16 in the four columns of one brick and 32, S - 1, S, 0 in those of the next: the
    mark falls on the first / last nibble of a word, in the word above, in the column's top word, or nowhere."""
    depth, S = 6, 64
    tris, want = [], np.zeros((S, S, S), np.uint8)
    cols = [(20, 20), (21, 20), (20, 21), (21, 21), (22, 20), (23, 20), (22, 21), (23, 21)]
    for (x, y), k in zip(cols, (1, 8, 9, 16, 32, S - 1, S, 0)):
        tris.append(sheet(x, y, x + 1, y + 1, k * U))
        want[x, y, :k] = 1
    tris = np.concatenate(tris)
    assert np.array_equal(M.xor_mesh(S, tris), want)
    assert np.array_equal(voxelised(depth, tris), want)
    check(depth, np.concatenate([tris, sheet(19, 19, 25, 23, 70 * U)]), "under a roof above the volume")


def test_two_crossings_at_one_voxel_cancel(built):
    """Two sheets that cross the same voxel of the same columns in one call toggle the same mark bit twice."""
    depth, S = 5, 32
    tris = np.concatenate([sheet(3, 4, 9, 11, 5 * U + 3), sheet(5, 2, 12, 8, 5 * U + 20), sheet(0, 0, 7, 7, 17 * U)])
    want = check(depth, tris, "cancelling sheets")
    assert not want[8, 7, :].any()                                      # under the two: the marks cancelled
    assert want[6, 6, :17].all() and not want[6, 6, 17:].any()          # under all three: the third alone is left
    assert not want[4, 5, :5].any() and want[4, 5, 5:17].all()          # the first and the third
    assert want[10, 3, :5].all() and not want[10, 3, 5:].any()          # the second alone


# ---- algebra that needs no model -----------------------------------------------------------------------------------

def test_algebra(built, heights):
    import cpuvoxelraycaster_amd as vrc
    import test_gpu_volume as V
    depth, S = 6, 64
    rng = np.random.default_rng(3)
    tris = np.concatenate([sphere(S, 19.4, (30.1, 27.9, 33.3)), tetrahedron(S, rng)])
    once = voxelised(depth, tris)
    assert 0 < once.sum() < S ** 3
    # order and winding
    t = tris[rng.permutation(len(tris))].reshape(-1, 3, 3)
    flip = rng.random(len(t)) < 0.5
    t[flip] = t[flip][:, ::-1, :]
    assert np.array_equal(voxelised(depth, t.reshape(-1, 9)), once)
    # twice = never; into a terrain volume = before ^ once
    terrain = V.terrain_volume(heights, depth)
    volume = vrc.VoxelVolume(depth)
    volume.setVoxels(np.argwhere(terrain))
    volume.xorMesh(tris)
    assert np.array_equal(volume.download(), terrain ^ once)
    volume.xorMesh(tris)
    assert np.array_equal(volume.download(), terrain)
    volume.close()
    # whole-voxel translation
    ball = sphere(S, 11.7, (20.3, 22.8, 19.6))
    base = voxelised(depth, ball)
    shift = np.array([13, -7, 21])
    moved = voxelised(depth, ball + np.tile(shift * U, 3).astype(np.int32))
    want = np.zeros_like(base)
    want[13:, :S - 7, 21:] = base[:S - 13, 7:, :S - 21]
    assert base[:, :7, :].sum() == 0 and np.array_equal(moved, want) and base.sum() == moved.sum() > 5000


def test_degenerate_and_out_of_range_triangles(built):
    depth, S = 5, 32
    roof = sheet(2, 2, 20, 20, 9 * U + 5)
    nothing = np.array([[0, 0, 0, 8 * U, 0, 0, 8 * U, 0, 8 * U],                  # vertical: n.z == 0
                        [U, U, U, U, U, U, U, U, U],                              # a point
                        [0, 0, 0, U, U, U, 2 * U, 2 * U, 2 * U],                  # a line
                        [3 * U, 3 * U, 3 * U, 9 * U, 9 * U, 6 * U, 3 * U, 3 * U, 3 * U]], np.int32)
    want = check(depth, np.concatenate([nothing, roof, nothing]), "degenerate")
    assert np.array_equal(want, M.xor_mesh(S, roof)) and want.sum() == 18 * 18 * 9
    assert not voxelised(depth, nothing).any()
    lim = 1 << 17
    far = np.array([[0, 0, 9 * U, lim + 1, 0, 9 * U, 0, 8 * U, 9 * U],
                    [0, 0, 9 * U, 8 * U, 0, 9 * U, 0, -lim - 1, 9 * U],
                    [0, 0, lim + 1, 8 * U, 0, 9 * U, 0, 8 * U, 9 * U]], np.int32)
    assert np.array_equal(check(depth, np.concatenate([far[:2], roof, far[2:]]), "out of range"), want)
    edge = np.array([[0, 0, 9 * U, lim, 0, 9 * U, 0, 8 * U, 9 * U], [0, 0, -lim, 8 * U, 0, lim, 0, 8 * U, lim]], np.int32)
    assert check(depth, edge, "at the limit").sum() > 0


def test_empty_call_and_memory_kinds(built):
    """n == 0 with and without a buffer; VRC_MEM_HOST and VRC_MEM_DEVICE give the same volume."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    volume = vrc.VoxelVolume(depth)
    volume.xorMesh(np.zeros((0, 9), np.int32))
    assert vrc.capi.load().vrc_volume_xor_mesh(volume._h, 0, None, vrc.capi.VRC_MEM_DEVICE, None) == 0
    assert volume.solidCount() == 0
    tris = sphere(S, 25.2, (31.3, 33.1, 28.8))
    t = torch.from_numpy(tris).cuda()
    torch.cuda.synchronize()
    volume.xorMesh((len(tris), t.data_ptr()), device=True)
    got = volume.download()
    assert np.array_equal(got, voxelised(depth, tris)) and np.array_equal(got, M.xor_mesh(S, tris))
    volume.close()


def test_ordered_behind_device_edits_and_before_commit(built):
    """A device-memory fill_boxes and a device-memory xor_mesh on one caller's stream, then commit with nothing in between:
    the mesh is XORed into the filled boxes, and the committed array is the host builder's for the model's occupancy."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    import test_gpu_volume as V
    depth, S = 6, 64
    boxes = np.array([[0, 0, 0, S, S, 20], [10, 10, 10, 40, 40, 60]], np.uint32)
    tris = sphere(S, 22.6, (30.2, 29.7, 31.4))
    t_boxes, t_tris = torch.from_numpy(boxes.view(np.int32)).cuda(), torch.from_numpy(tris).cuda()
    torch.cuda.synchronize()
    volume = vrc.VoxelVolume(depth)
    with Stream() as stream:
        volume.fillBoxesDevice(len(boxes), t_boxes.data_ptr(), True, stream)
        volume.xorMesh((len(tris), t_tris.data_ptr()), device=True, stream=stream)
        nodes = V.committed(volume)
    want = np.zeros((S, S, S), np.uint8)
    for x0, y0, z0, x1, y1, z1 in boxes.astype(np.int64):
        want[x0:x1, y0:y1, z0:z1] = 1
    M.xor_mesh(S, tris, want)
    assert np.array_equal(volume.download(), want)
    assert same(nodes, V.expected_nodes(want, depth))
    volume.close()


def test_scratch_does_not_grow_and_stays_zero(built):
    """Twenty calls at 64^3: the volume's own scratch (vrc_volume_edit_scratch_bytes) is nothing before the first call, the
    mark field (one byte per brick, 32 KiB) plus the staged triangles after it, and the same after every later call.  The
    mark field is zero afterwards: the next call, an open sheet, still gives the model's result."""
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    rng = np.random.default_rng(20)
    volume = vrc.VoxelVolume(depth)
    assert volume.editScratchBytes() == 0
    want = np.zeros((S, S, S), np.uint8)
    held = []
    for i in range(20):
        tris = sphere(S, rng.uniform(5, 40), rng.uniform(10, 54, 3), 1) if i % 2 else tetrahedron(S, rng)
        volume.xorMesh(tris)
        M.xor_mesh(S, tris, want)
        held.append(volume.editScratchBytes())
    # the staging block holds the largest host-memory batch so far: 4 triangles of 36 bytes, then 80
    assert held == [S ** 3 // 8 + 4 * 36] + [S ** 3 // 8 + 80 * 36] * 19, held
    roof = sheet(-3, 5, 50, 70, 37 * U + 11)
    volume.xorMesh(roof)
    M.xor_mesh(S, roof, want)
    assert np.array_equal(volume.download(), want)
    volume.close()


# ---- the two launch shapes -----------------------------------------------------------------------------------------

def test_many_small_items(built):
    """5 000 one-voxel tetrahedra (20 000 triangles) in one call: one workgroup per triangle."""
    depth, S = 6, 64
    rng = np.random.default_rng(5)
    corner = rng.integers(-1, S, (5000, 1, 3)) * U
    v = corner + rng.integers(0, U + 1, (5000, 4, 3))                     # inside one voxel's cube, overlapping others'
    faces = np.array([(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)])
    tris = v[:, faces, :].reshape(-1, 9).astype(np.int32)
    assert len(tris) == 20000
    want = check(depth, tris, "5000 tetrahedra")
    assert want.sum() > 50


def test_one_item_split_over_many_workgroups(built):
    """One box mesh spanning the 64^3 volume: 12 triangles of 4096 columns each, every one split over several workgroups."""
    depth, S = 6, 64
    want = check(depth, box((0, 0, 0), (S, S, S)), "spanning box")
    assert want.all()
    want = check(depth, box((-5.5, -1, 0.5), (S + 3, S - 0.5, S - 1.5)), "spanning box, off the grid")
    assert want.sum() > S ** 3 * 0.9


# ---- the user's story ----------------------------------------------------------------------------------------------

def test_stamp_a_model_into_the_terrain_and_render(built, heights, textures):
    """stampMesh: an icosphere through a 32^3 clipboard into the 128^3 terrain with OR at an odd offset; the committed scene
    is the host builder's array for terrain | model's ball, and a 64 x 64 frame of it is the oracle's."""
    import cpuvoxelraycaster_amd as vrc
    import test_gpu_volume as V
    depth, S, W, Hh = 7, 128, 64, 64
    terrain = V.terrain_volume(heights, depth)
    scene = vrc.LSVO.fromTerrain(heights, depth, textures=textures)
    volume = vrc.VoxelVolume.fromScene(scene)
    verts, faces = vrc.icosphere(2)
    radius, centre = 14.6, (61.3, 83.9, 40.2)                          # half in the ground, in front of the camera
    lo, size = volume.stampMesh(verts, faces, vrc.capi.VRC_COPY_OR, radius, centre)
    assert lo == (46, 69, 25) and size == (30, 30, 30)                     # a 32^3 clipboard; odd offsets in y and z, an even one in x
    ball = M.xor_mesh(S, M.soup(M.quantise(verts, radius, centre), faces))
    want = terrain | ball
    assert (ball & terrain).any() and (ball & (1 - terrain)).sum() > 3000
    assert np.array_equal(volume.download(), want)
    after = volume.commit()
    nodes = after.downloadNodes()
    assert same(nodes, vrc.build_volume_lsvo(want, depth))
    cam, light = vrc.reference_camera(depth, pitch=-0.5), vrc.reference_light(depth)
    rc = vrc.RayCaster(after, (W, Hh))
    rc.setLightPosition(light)
    rc.use_gi = rc.use_samples = True
    rc.shadow_samples = 1
    rc.renderFrame(cam, spp=1)
    want_acc, stats = V.oracle_frame(nodes, depth, textures, cam, light, W, Hh, 1)
    assert np.array_equal(rc.readAccum(), want_acc) and V.stats_tuple(rc.stats()) == stats
    bare, _ = V.oracle_frame(scene.downloadNodes(), depth, textures, cam, light, W, Hh, 1)
    assert (want_acc != bare).any(axis=2).sum() > 500                      # the ball is in the picture
    for v in (rc, after, volume, scene):
        v.close()


def test_voxelised_sphere_has_no_holes(built):
    """An EMPTY flood from a corner of a lone voxelised sphere at 64^3 leaves exactly the sphere's complement: the solid is
    watertight and has no cavity, checked through an existing operation."""
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    verts, faces = vrc.icosphere(3)
    medium = vrc.VoxelVolume(depth)
    medium.voxelizeMesh(verts, faces, 24.3, (31.7, 32.2, 30.9))
    ball = medium.download()
    assert np.array_equal(ball, M.xor_mesh(S, M.soup(M.quantise(verts, 24.3, (31.7, 32.2, 30.9)), faces))) and ball.sum() > 50000
    air = vrc.VoxelVolume(depth)
    air.setVoxels([[0, 0, 0]])
    st = air.flood(medium, 6, True)
    assert st.converged == 1 and st.reached == S ** 3 - int(ball.sum())
    assert np.array_equal(air.download(), 1 - ball)
    air.close()
    medium.close()
