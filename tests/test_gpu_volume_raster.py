"""Surface voxelisation on the GPU (vrc_raster_mesh): every download is compared bit for bit with the numpy model
(raster_model.py), in both modes, setting into an empty volume and clearing from a full one, at the smallest shapes at which
each mechanism of the kernels can break; then the memory forms, the ordering, the scratch blocks and the compositions."""
import numpy as np
import pytest

import raster_model as model
import voxelize_model
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu

U = model.UNIT
MODES = (model.TOUCHED, model.THIN)


def on_device(arr, dtype=np.int32):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype).view(np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def hold_to_model(depth, tris, expect_some=True, expect_thin=None):
    """both modes, set into an empty volume and cleared from a full one, against the model"""
    S = 1 << depth
    tris = np.asarray(tris, np.int64).reshape(-1, 9)
    for mode in MODES:
        sel = model.selected(S, tris, mode)
        assert sel.any() == (expect_some if mode == model.TOUCHED or expect_thin is None else expect_thin), mode
        for solid in (True, False):
            volume = volume_of(np.zeros((S, S, S), np.uint8))
            if not solid:
                volume.fillBoxes([(0, 0, 0, S, S, S)])
            volume.rasterMesh(tris, mode, solid)
            want = np.full((S, S, S), 0 if solid else 1, np.uint8)
            want[sel] = 1 if solid else 0
            got = volume.download()
            volume.close()
            assert np.array_equal(got, want), (depth, mode, solid, int((got != want).sum()))


# ---- 1. depths ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3, 5])
def test_mixed_triangles(built, depth):
    """depth 2: two brick columns share a word of the occupancy"""
    S = 1 << depth
    rng = np.random.default_rng(700 + depth)
    tris = np.concatenate([rng.integers(-U, U * S + U, (12, 9)), model.small_triangles(rng, S, 40),
                           32 * rng.integers(-1, 2 * S + 2, (12, 9))])      # vertices on multiples of 64 and on + 32
    hold_to_model(depth, tris)


# ---- 2. clipping ---------------------------------------------------------------------------------------------------------

def test_clipping_at_64(built):
    """one triangle larger than the volume on every side, negative coordinates, and one wholly outside"""
    S = 64
    far = U * S
    hold_to_model(6, [[-2 * far, -far, 900, 3 * far, -far, 1700, far // 2, 3 * far, 2500]])
    hold_to_model(6, [[-700, -300, -90, 1500, -200, 800, -100, 2100, 40], [-5000, 100, 100, 640, 100, 100, 640, 100, 100]])
    hold_to_model(6, [[far + 65, 0, 0, far + 900, 64, 0, far + 65, 500, 300], [0, -65, 0, far, -65, 0, 0, -65, far],
                      [100, 100, -3000, 900, 100, -2000, 100, 900, -1000]], expect_some=False)
    L = model.LIMIT
    hold_to_model(6, [[-L, -L, -L, L, L, L, L, -L, 0], [L + 1, 0, 0, 0, far, 0, 0, 0, far]])     # the limit itself; the second is dropped


# ---- 3. the launch shapes ----------------------------------------------------------------------------------------------

def test_a_lone_triangle_at_128(built):
    """the corner-to-corner triangle alone gets the full blockIdx.y split: 64 workgroups of 256 threads for its 128 x 128 columns"""
    hold_to_model(7, model.corner_triangle(128))


def test_the_strided_loop_runs_more_than_once(built):
    """300 triangles at 64^3 get ceil(4096 / 300) = 14 workgroups each, 3584 threads, and a triangle that spans the volume has up
    to 64 x 64 = 4096 columns: its threads come round a second time"""
    S = 64
    far = U * S
    spanning = np.concatenate([model.corner_triangle(S), [[0, far, 17, far, 0, 900, far, far, 3001], [5, 0, 0, 70, far, far, 3000, 0, far],
                                                           [0, 77, far, far, 2000, 0, far, 1000, far]]])
    tris = np.concatenate([model.small_triangles(np.random.default_rng(77), S, 296), spanning])
    hold_to_model(6, tris)


def test_one_workgroup_per_triangle_above_4096(built):
    S = 32
    tris = model.small_triangles(np.random.default_rng(55), S, 5000)
    hold_to_model(5, tris)


# ---- 4. the fixed cases of the host test -------------------------------------------------------------------------------

def test_fixed_cases(built):
    hold_to_model(4, model.box_mesh(U * np.array([3, 4, 5]), U * np.array([7, 6, 11])))
    hold_to_model(4, model.box_mesh(U * np.array([-2, 5, 5]), U * np.array([4, 9, 20])))
    for k in (0, 1, 5, 16, 20):
        S = 16
        t = [0, 0, 0] + [U * k] * 6
        volume = volume_of(np.zeros((S, S, S), np.uint8))
        volume.rasterMesh([t], model.TOUCHED)
        got = volume.download()
        volume.close()
        assert np.array_equal(got.astype(bool), model.selected(S, [t], model.TOUCHED)) and got.any(), k
    hold_to_model(4, [[0, 0, 0, 320, 320, 320, 320, 320, 320], [64, 900, 64, 64, 100, 64, 64, 500, 64]], expect_thin=False)    # segments
    hold_to_model(4, [[U * 7, 30, 50, U * 7, 900, 100, U * 7, 400, 1000], [100, U * 3 + 32, 90, 800, U * 3 + 32, 200, 300, U * 3 + 32, 990],
                      [0, 0, 1024, 1024, 0, 1024, 0, 1024, 1024]])          # a boundary plane, a centre plane, the volume's own face


# ---- 5. memory forms, ordering, scratch ------------------------------------------------------------------------------

def test_device_form_on_a_stream_equals_the_host_form(built):
    S = 32
    tris = model.small_triangles(np.random.default_rng(8), S, 300).astype(np.int32)
    for mode in MODES:
        a, b = volume_of(np.zeros((S, S, S), np.uint8)), volume_of(np.zeros((S, S, S), np.uint8))
        with Stream() as stream:
            t = on_device(tris)
            a.rasterMesh(tris, mode)
            b.rasterMesh((len(tris), t.data_ptr()), mode, True, device=True, stream=stream)
            got_a, got_b = a.download(), b.download()                         # download waits for the stream's edit
            del t
        a.close()
        b.close()
        assert np.array_equal(got_a, got_b) and np.array_equal(got_a.astype(bool), model.selected(S, tris, mode))


def test_ordered_behind_an_asynchronous_fill(built):
    S = 64
    tris = np.random.default_rng(9).integers(0, U * S, (30, 9)).astype(np.int32)
    box = np.array([[5, 0, 9, 60, 64, 50]], np.uint32)
    for mode in MODES:
        volume = volume_of(np.zeros((S, S, S), np.uint8))
        with Stream() as stream:
            b, t = on_device(box, np.uint32), on_device(tris)
            volume.fillBoxesDevice(1, b.data_ptr(), True, stream)
            volume.rasterMesh((len(tris), t.data_ptr()), mode, False, device=True, stream=stream)
            got = volume.download()
            del b, t
        volume.close()
        want = np.zeros((S, S, S), np.uint8)
        want[5:60, 0:64, 9:50] = 1
        sel = model.selected(S, tris, mode)
        assert (want[sel] == 1).any()
        want[sel] = 0
        assert np.array_equal(got, want), mode


def test_no_scratch_block(built):
    S = 32
    volume = volume_of(np.zeros((S, S, S), np.uint8))                         # fresh: no call has run on it
    tris = model.small_triangles(np.random.default_rng(10), S, 100)
    before = volume.editScratchBytes()
    with Stream() as stream:
        t = on_device(tris)
        for mode in MODES:
            volume.rasterMesh((len(tris), t.data_ptr()), mode, True, device=True, stream=stream)
        assert volume.solidCount() > 0
        del t
    assert volume.editScratchBytes() == before
    # the host form stages its list as vrc_volume_fill_spheres does, through the staging block every such call shares
    volume.fillSpheres([(1, 1, 1, 0)] * (len(tris) * 9 // 4 + 1))
    staged = volume.editScratchBytes()
    volume.rasterMesh(tris, model.TOUCHED)
    assert volume.editScratchBytes() == staged
    volume.close()


# ---- 6. compositions ---------------------------------------------------------------------------------------------------

BOX_VERTS = np.array([(x, y, z) for x in (3.3, 12.6) for y in (2.5, 9.25) for z in (4.0, 13.9)], np.float64)
BOX_FACES = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                      (1, 5, 7), (1, 7, 3)], np.int64)


def test_solid_from_shell(built):
    """a closed box: the solid is xor_mesh's united with the thin shell; one triangle listed twice changes nothing, where xorMesh
    of that list inverts columns"""
    import cpuvoxelraycaster_amd as vrc
    S = 16
    fixed = vrc.VoxelVolume.quantiseMesh(BOX_VERTS)
    tris = fixed[BOX_FACES].reshape(-1, 9)
    want = voxelize_model.xor_mesh(S, tris).astype(bool) | model.selected(S, tris, model.THIN)
    assert 0 < int(want.sum()) < S ** 3 and int(voxelize_model.xor_mesh(S, tris).sum()) > 0
    doubled = np.concatenate([BOX_FACES, BOX_FACES[8:9]])                     # a triangle of the face z = 4.0: xor_mesh reads along z
    for faces in (BOX_FACES, doubled):
        volume = vrc.VoxelVolume(4)
        volume.solidFromShell(BOX_VERTS, faces)
        got = volume.download().astype(bool)
        volume.close()
        assert np.array_equal(got, want), len(faces)
    volume = vrc.VoxelVolume(4)
    volume.voxelizeMesh(BOX_VERTS, doubled)
    broken = volume.download().astype(bool)
    volume.close()
    assert not np.array_equal(broken, voxelize_model.xor_mesh(S, tris).astype(bool))
    # an existing world is kept: the solid is ORed in
    world = np.zeros((S, S, S), np.uint8)
    world[0:2, :, :] = 1
    volume = volume_of(world)
    volume.solidFromShell(BOX_VERTS, BOX_FACES)
    got = volume.download().astype(bool)
    volume.close()
    assert np.array_equal(got, want | world.astype(bool))


def test_shell_mesh_goes_through_quantise(built):
    import cpuvoxelraycaster_amd as vrc
    S = 16
    for thin in (False, True):
        volume = vrc.VoxelVolume(4)
        volume.shellMesh(BOX_VERTS, BOX_FACES, thin, True, 0.5, (2.0, 3.0, 1.5))
        got = volume.download().astype(bool)
        volume.close()
        tris = voxelize_model.soup(voxelize_model.quantise(BOX_VERTS, 0.5, (2.0, 3.0, 1.5)), BOX_FACES)
        assert np.array_equal(got, model.selected(S, tris, model.THIN if thin else model.TOUCHED)) and got.any()


def test_round_trip_renders(built):
    """toMesh -> THIN -> commit -> one batch of rays"""
    import cpuvoxelraycaster_amd as vrc
    S = 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[6:26, 8:20, 5:27] = 1
    vol[10:14, 8:30, 10:14] = 1
    source = volume_of(vol)
    verts, quads = source.toMesh(closed=True)
    source.close()
    tris = (verts.astype(np.int64) * U)[quads[:, [0, 1, 2, 0, 2, 3]]].reshape(-1, 9)
    shell = vrc.VoxelVolume(5)
    shell.rasterMesh(tris, model.THIN)
    got = shell.download().astype(bool)
    assert np.array_equal(got, model.selected(S, tris, model.THIN)) and got.any()
    scene = shell.commit()
    shell.close()
    n = 256
    g = (np.arange(n) % 16 + 0.5) / 16.0, (np.arange(n) // 16 + 0.5) / 16.0
    org = np.stack([1.0 + g[0], np.full(n, 0.9), 1.0 + g[1]], -1).astype(np.float32)
    d = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (n, 1))
    hits = scene.castRays(org, d)
    scene.close()
    assert len(hits) == n and int(((hits["hit"] & 0xff) == 1).sum()) > 20
