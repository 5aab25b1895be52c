"""The capsule brush of the C++ host adapter (HipVoxelVolume::strokeAtHits, fillPolyline, fillLine) compiled with plain g++
against the C ABI and run on the GPU: cast -> stroke at hits -> polyline -> line -> stroke must leave, step by step, the solid
counts and the sparse tile streams that the same sequence leaves through the Python VoxelVolume."""
import re

import numpy as np
import pytest

from stroke_model import scan_rays
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_strokes_match_python_path(built, tmp_path):
    import cpuvoxelraycaster_amd as vrc
    depth, radius, max_gap, pipe = 7, 2, 9, 1
    org, d = scan_rays(depth, 120, 4.0)
    np.concatenate([org, d], axis=1).astype(np.float32).tofile(tmp_path / "rays.bin")
    points = np.array([(10, 30, 12), (100, 35, 20), (110, 38, 115), (-5, 40, 90), (64, 20, 64)], np.int32)
    points.tofile(tmp_path / "points.bin")

    out = run_cpp_main(tmp_path, "voxel_stroke_main", depth, tmp_path / "rays.bin", radius, max_gap, tmp_path / "points.bin", pipe)
    m = re.search(r"rays=(\d+) unit_hits=(\d+) solid=(\d+) dug=(\d+):([0-9a-f]{16}) piped=(\d+):([0-9a-f]{16}) lined=(\d+):([0-9a-f]{16}) "
                  r"built=(\d+):([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    g = m.groups()
    got = [int(v) for v in g[:4]] + [int(g[4], 16), int(g[5]), int(g[6], 16), int(g[7]), int(g[8], 16), int(g[9]), int(g[10], 16)]

    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    hits = scene.castRays(org, d)
    volume = vrc.VoxelVolume.fromScene(scene)
    want = [len(org), int(((hits["hit"] & 0xff) == 1).sum()), volume.solidCount()]

    def step():
        want.extend([volume.solidCount(), fnv1a(volume.pack().tobytes())])

    volume.strokeAtHits(hits, radius, False, max_gap)
    step()
    volume.fillPolyline(points, pipe, True, closed=True)
    step()
    volume.fillLine(points[0], points[1], 0, False)
    step()
    volume.strokeAtHits(hits, 0, True)
    step()
    assert want[1] > 50 and want[3] < want[2] and want[5] > want[3] and want[7] < want[5] and want[9] > want[7]   # every step changed the volume
    assert got == want
