"""The mesh voxelisation of the C++ host adapter (HipVoxelVolume::xorMesh / voxelizeMesh / stampMesh) compiled with plain g++
against the C ABI and run on the GPU at 64^3: the three occupancies it writes equal the numpy model's, bit for bit."""
import numpy as np
import pytest

import voxelize_model as M
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_mesh_methods_match_the_model(built, tmp_path):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    scale, off = 17.3, (30.2, 25.7, 33.1)
    verts, faces = vrc.icosphere(2)
    rng = np.random.default_rng(11)
    box_verts, box_faces = vrc.box_mesh((3.5, -4, 10), (40, 20.5, 70))
    tris = M.soup(M.quantise(box_verts), box_faces)
    tris = np.concatenate([tris, rng.integers(-5 * 64, 70 * 64, (40, 9)).astype(np.int32)])      # and an open soup on top
    verts.astype(np.float64).tofile(tmp_path / "verts.bin")
    faces.astype(np.uint32).tofile(tmp_path / "faces.bin")
    tris.tofile(tmp_path / "tris.bin")

    out = run_cpp_main(tmp_path, "voxel_mesh_main", depth, tmp_path / "verts.bin", tmp_path / "faces.bin", tmp_path / "tris.bin",
                       repr(scale), repr(off[0]), repr(off[1]), repr(off[2]), tmp_path / "out")

    def got(name):
        return np.fromfile(tmp_path / f"out_{name}.bin", np.uint8).reshape(S, S, S)

    want = np.zeros((S, S, S), np.uint8)
    want[1, 2, 3] = 1
    M.xor_mesh(S, tris, want)
    assert np.array_equal(got("xor"), want)

    ball = M.xor_mesh(S, M.soup(M.quantise(verts, scale, off), faces))
    assert ball.sum() > 15000
    assert np.array_equal(got("vox"), ball)

    world = np.zeros((S, S, S), np.uint8)
    world[:, :S // 4, :] = 1
    world |= ball
    carve = M.xor_mesh(S, M.soup(M.quantise(verts, scale, (off[0] + 7.0, off[1] - 3.0, off[2] + 4.5)), faces))
    world &= 1 - carve
    assert (ball & carve).any() and (ball & (1 - carve)).any()
    assert np.array_equal(got("stamp"), world)
