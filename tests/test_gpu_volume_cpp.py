"""The write half of the C++ host adapter (HipVoxelVolume, HipRayCaster::setScene) compiled with plain g++ against the
C ABI and run on the GPU: setCell x N + commit + setScene must show the image the Python path renders."""
import os
import re

import numpy as np
import pytest

from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_voxel_volume_matches_python_path(built, tmp_path):
    import cpuvoxelraycaster_amd as vrc
    depth, W, H = 8, 160, 90
    S = 1 << depth
    golden = os.path.join(ROOT, "tests", "golden")
    bmps = [os.path.join(golden, "grass_top_16x16.bmp"), os.path.join(golden, "grass_side_16x16.bmp")]
    textures = vrc.load_textures_bmp(*bmps)
    # the edits: a pit under the crosshair (clears), a pillar next to it (sets), a few voxels outside the volume
    scene = vrc.LSVO.fromFastNoiseTerrain(depth, textures=textures)
    cam = vrc.reference_camera(depth, pitch=-0.5)
    org = np.array(tuple(cam.position), np.float32) / np.float32(S) + np.float32(1.0)
    rot = np.array(tuple(cam.rot), np.float32)
    voxel, _ = vrc.hit_to_voxel(depth, scene.castRay(org, [rot[2], rot[5], rot[8]]))
    g = np.mgrid[-6:7, -6:7, -6:7].reshape(3, -1).T
    pit = np.array(voxel) + g[(g ** 2).sum(1) <= 36]
    pillar = np.array(voxel) + np.array([(10, dy, 0) for dy in range(-30, 3)])
    edits = np.concatenate([np.c_[pit, np.zeros(len(pit), int)], np.c_[pillar, np.ones(len(pillar), int)],
                            [(S, 1, 1, 1), (1, S + 7, 1, 0)], np.c_[pit[:20], np.zeros(20, int)]]).astype(np.uint32)
    edits.tofile(tmp_path / "edits.bin")

    out = run_cpp_main(tmp_path, "voxel_volume_main", depth, tmp_path / "edits.bin", bmps[0], bmps[1], W, H, tmp_path / "out.rgba", flags=())
    m = re.search(r"edits=(\d+) solid_before=(\d+) solid_after=(\d+) nodes_after=(\d+) changed=1 build_ms_positive=1", out.stdout)
    assert m, out.stdout
    got = np.fromfile(tmp_path / "out.rgba", np.uint8).reshape(H, W, 4)

    # the Python path: the same edits as batches, in the same order
    volume = vrc.VoxelVolume.fromScene(scene)
    before = volume.solidCount()
    i = 0
    while i < len(edits):
        j = i
        while j < len(edits) and edits[j, 3] == edits[i, 3]:
            j += 1
        volume.setVoxels(edits[i:j, :3], bool(edits[i, 3]))
        i = j
    after = volume.commit()
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) == (len(edits), before, volume.solidCount(), after.n_nodes)
    rc = vrc.RayCaster(scene, (W, H))
    rc.setLightPosition(vrc.reference_light(depth))
    rc.use_gi = rc.use_samples = True
    rc.renderFrame(cam, spp=2)
    rc.resetSamples()
    rc.setScene(after)
    rc.frame_index = 0
    rc.renderFrame(cam, spp=2)
    rc.samples_to_image()
    assert np.array_equal(rc.readImage(), got)
