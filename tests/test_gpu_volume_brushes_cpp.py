"""The brushes of the C++ host adapter (HipLSVO::castRaysRecords, HipVoxelVolume::fillSpheresAtHits) compiled with plain
g++ against the C ABI and run on the GPU: cast -> brush at hits -> commit -> setScene -> frame must show the image the same
sequence renders through the Python VoxelVolume."""
import os
import re

import numpy as np
import pytest

import raygen
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_brush_at_hits_matches_python_path(built, tmp_path):
    import cpuvoxelraycaster_amd as vrc
    depth, W, H, dig, build = 8, 160, 90, 4, 1
    golden = os.path.join(ROOT, "tests", "golden")
    bmps = [os.path.join(golden, "grass_top_16x16.bmp"), os.path.join(golden, "grass_side_16x16.bmp")]
    org, d = raygen.camera_rays(depth, 48, 27, -0.5)
    S = np.float32(1 << depth)
    org[:] = np.array(vrc.reference_camera_position(depth), np.float32) / S + np.float32(1.0)   # the camera the frame is rendered from
    np.concatenate([org, d], axis=1).astype(np.float32).tofile(tmp_path / "rays.bin")

    out = run_cpp_main(tmp_path, "voxel_brushes_main", depth, tmp_path / "rays.bin", bmps[0], bmps[1], W, H, dig, build)
    m = re.search(r"rays=(\d+) unit_hits=(\d+) solid_before=(\d+) solid_dug=(\d+) solid_after=(\d+) nodes_after=(\d+) image_hash=([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    got = [int(g) for g in m.groups()[:6]] + [int(m.group(7), 16)]

    scene = vrc.LSVO.fromFastNoiseTerrain(depth, textures=vrc.load_textures_bmp(*bmps))
    hits = scene.castRays(org, d)
    volume = vrc.VoxelVolume.fromScene(scene)
    want = [len(org), int(((hits["hit"] & 0xff) == 1).sum()), volume.solidCount()]
    volume.fillSpheresAtHits(hits, dig, False)
    want.append(volume.solidCount())
    volume.fillSpheresAtHits(hits, build, True)
    after = volume.commit()
    want += [volume.solidCount(), after.n_nodes]
    rc = vrc.RayCaster(scene, (W, H))
    rc.setLightPosition(vrc.reference_light(depth))
    rc.use_gi = rc.use_samples = True
    rc.setScene(after)
    rc.renderFrame(vrc.reference_camera(depth, pitch=-0.5), spp=2)
    rc.samples_to_image()
    want.append(fnv1a(rc.readImage().tobytes()))
    assert want[1] > 100 and want[3] < want[2] and want[4] > want[3]     # rays hit, the dig removed voxels, the build added some
    assert got == want
