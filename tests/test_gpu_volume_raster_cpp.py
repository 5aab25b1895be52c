"""Surface voxelisation through the C++ host adapter (HipVoxelVolume::rasterMesh, shellMesh) compiled with plain g++ against the
C ABI and run on the GPU: touched voxels set, a thin shell carved out of a full volume, an indexed mesh's skin set and partly
cleared again must leave the solid counts and the sparse tile streams of the numpy model's volumes."""
import re

import numpy as np
import pytest

import raster_model as model
import voxelize_model
from volume_support import fnv1a, run_cpp_main, volume_of

pytestmark = pytest.mark.gpu

VERTS = np.array([(x, y, z) for x in (3.3, 12.6) for y in (2.5, 9.25) for z in (4.0, 13.9)], np.float64)
FACES = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], np.uint32)


def test_cpp_raster_matches_the_model(built, tmp_path):
    depth, S, scale, offset = 5, 32, 1.5, 2.25
    rng = np.random.default_rng(21)
    tris = np.concatenate([model.small_triangles(rng, S, 150), rng.integers(-64, 64 * S + 64, (10, 9))]).astype(np.int32)
    tris.tofile(tmp_path / "tris.bin")
    VERTS.tofile(tmp_path / "verts.bin")
    FACES.tofile(tmp_path / "faces.bin")
    out = run_cpp_main(tmp_path, "voxel_raster_main", depth, tmp_path / "tris.bin", tmp_path / "verts.bin", tmp_path / "faces.bin", scale, offset)
    m = re.search(r"triangles=(\d+) touched=(\d+):([0-9a-f]{16}) carved=(\d+):([0-9a-f]{16}) skin=(\d+):([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    g = m.groups()
    got = [int(g[0]), int(g[1]), int(g[2], 16), int(g[3]), int(g[4], 16), int(g[5]), int(g[6], 16)]

    touched = model.raster_mesh(S, tris, model.TOUCHED)
    carved = model.raster_mesh(S, tris, model.THIN, 0, np.ones((S, S, S), np.uint8))
    skin = model.raster_mesh(S, voxelize_model.soup(voxelize_model.quantise(VERTS, scale, (offset,) * 3), FACES), model.THIN)
    model.raster_mesh(S, voxelize_model.soup(voxelize_model.quantise(VERTS, scale, (offset + 3.0, offset, offset)), FACES), model.TOUCHED, 0, skin)
    want = [len(tris)]
    for field in (touched, carved, skin):
        volume = volume_of(field)
        want.extend([int(field.sum(dtype=np.int64)), fnv1a(volume.pack().tobytes())])
        volume.close()
    assert 0 < want[1] < S ** 3 and want[3] < S ** 3 and 0 < want[5]
    assert got == want
