"""The surface extraction of the C++ host adapter (HipVoxelVolume::surfaceCount / surfaceFaces / surfaceTriangles / toObj)
compiled with plain g++ against the C ABI and run on the GPU at 64^3: two spheres and a carved box; the triangles voxelised
back with xorMesh give the same volume (the XOR of both counts 0 voxels), the figures equal the numpy model's and the OBJ
file holds one `f` line per face and one `v` line per distinct corner."""
import re

import numpy as np
import pytest

import surface_model as F
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_surface_round_trip_and_obj(built, tmp_path):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    obj = tmp_path / "world.obj"
    out = run_cpp_main(tmp_path, "voxel_surface_main", depth, obj)
    m = re.search(r"solid=(\d+) back=(\d+) differ=(\d+) total=(\d+) open=(\d+) faces=(\d+) triangles=(\d+) window=(\d+) obj_faces=(\d+)", out.stdout)
    assert m, out.stdout
    solid, back, differ, total, open_total, n_faces, n_tris, window, obj_faces = (int(g) for g in m.groups())

    # the same scene through the model
    g = np.indices((S, S, S)).astype(np.int64)
    V = np.zeros((S, S, S), np.uint8)
    for (cx, cy, cz), r in (((S // 3, S // 2, S // 2), S // 4), ((S - 3, S // 2 + 5, 4), S // 5)):
        V |= ((g[0] - cx) ** 2 + (g[1] - cy) ** 2 + (g[2] - cz) ** 2 <= r * r).astype(np.uint8)
    V[S // 4:S // 2, S // 2 - 3:S // 2 + 4, :] = 0
    faces = F.faces(V, True)
    assert solid == int(V.sum()) > 10000 and back == solid and differ == 0
    assert total == n_faces == obj_faces == faces.shape[0] and n_tris == 2 * n_faces and window == 1
    assert open_total == F.faces(V, False).shape[0] < total                   # the second sphere leaves the volume

    verts, quads = vrc.VoxelVolume.meshFromFaces(faces)
    lines = obj.read_text().splitlines()
    v = np.array([[int(q) for q in line.split()[1:]] for line in lines if line.startswith("v ")], np.int32)
    f = np.array([[int(q) for q in line.split()[1:]] for line in lines if line.startswith("f ")], np.int64)
    assert len(lines) == len(v) + len(f) and np.array_equal(v, verts) and np.array_equal(f - 1, quads)
