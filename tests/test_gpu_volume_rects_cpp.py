"""The merged-rectangle extraction of the C++ host adapter (HipVoxelVolume::rectCount / surfaceRects / rectTriangles /
toObj(merged)) compiled with plain g++ against the C ABI and run on the GPU at 32^3: a sphere, a box on two walls and a
carved slot.  The records, the triangles and the OBJ file equal the numpy model's (tests/rect_model.py), and the triangles
voxelised back with xorMesh give the same volume."""
import re

import numpy as np
import pytest

import rect_model as R
import surface_model as F
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_rects_round_trip_and_obj(built, tmp_path):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 5, 32
    obj = tmp_path / "world.obj"
    out = run_cpp_main(tmp_path, "voxel_rects_main", depth, obj)
    head, rect_line, tri_line = out.stdout.splitlines()
    print(head)
    m = re.search(r"solid=(\d+) back=(\d+) differ=(\d+) total=(\d+) open=(\d+) faces=(\d+) rects=(\d+) triangles=(\d+) window=(\d+) obj_faces=(\d+)", head)
    assert m, head
    solid, back, differ, total, open_total, n_faces, n_rects, n_tris, window, obj_faces = (int(g) for g in m.groups())

    # the same scene through the model
    g = np.indices((S, S, S)).astype(np.int64)
    V = ((g[0] - S // 3) ** 2 + (g[1] - S // 2) ** 2 + (g[2] - S // 2) ** 2 <= (S // 4) ** 2).astype(np.uint8)
    V[S // 2:S - 3, 2:S // 3, :] = 1
    V[S // 4:S // 2, S // 2 - 1:S // 2 + 2, :] = 0
    want = R.rects(V, True)
    assert solid == int(V.sum()) > 2000 and back == solid and differ == 0
    assert n_faces == F.faces(V, True).shape[0] > total
    assert total == n_rects == obj_faces == want.shape[0] and n_tris == 2 * n_rects and window == 1
    assert open_total == R.rects(V, False).shape[0] < total
    assert np.array_equal(np.array(rect_line.split()[1:], np.uint32).reshape(-1, 4), want)
    assert np.array_equal(np.array(tri_line.split()[1:], np.int32).reshape(-1, 9), R.triangles(want))

    verts, quads = vrc.VoxelVolume.meshFromFaces(want, merged=True)
    lines = obj.read_text().splitlines()
    v = np.array([[int(q) for q in line.split()[1:]] for line in lines if line.startswith("v ")], np.int32)
    f = np.array([[int(q) for q in line.split()[1:]] for line in lines if line.startswith("f ")], np.int64)
    assert len(lines) == len(v) + len(f) and np.array_equal(v, verts) and np.array_equal(f - 1, quads)
