"""The flood of the C++ host adapter (HipVoxelVolume::flood / keepConnected) compiled with plain g++ against the C ABI and run
on the GPU at 128^3: cast -> dig at hits -> flood of the air -> keepConnected -> commit -> setScene -> frame must give the
counts and the image the same sequence gives through the Python VoxelVolume, and the counts of the numpy model."""
import re

import numpy as np
import pytest

import flood_model
import raygen
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("connectivity", [6, 26])
def test_cpp_flood_matches_python_path_and_model(built, tmp_path, connectivity):
    import cpuvoxelraycaster_amd as vrc
    depth, S, W, H, dig = 7, 128, 160, 90, 5
    org, d = raygen.camera_rays(depth, 48, 27, -0.5)
    np.concatenate([org, d], axis=1).astype(np.float32).tofile(tmp_path / "rays.bin")

    out = run_cpp_main(tmp_path, "voxel_flood_main", depth, tmp_path / "rays.bin", W, H, dig, connectivity)
    m = re.search(r"rays=(\d+) solid_dug=(\d+) air=(\d+) air_converged=(\d+) supported=(\d+) debris=(\d+) nodes_after=(\d+) image_hash=([0-9a-f]{16})", out.stdout)
    assert m, out.stdout
    got = [int(g) for g in m.groups()[:7]] + [int(m.group(8), 16)]

    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    hits = scene.castRays(org, d)
    volume = vrc.VoxelVolume.fromScene(scene)
    volume.fillSpheresAtHits(hits, dig, False)
    volume.fillBoxes([[20, S // 2 - 5, 20, 23, S // 2 - 2, 23]])
    dug = volume.download()
    want = [len(org), int(dug.sum())]
    air = vrc.VoxelVolume(depth)
    air.fillBoxes([[0, S - 1, 0, S, S, S]])
    st = air.flood(volume, connectivity, True)
    want += [st.reached, st.converged]
    anchors = [[0, S // 2 + 1, 0, S, S // 2 + 2, S]]
    debris = volume.keepConnected(anchors, connectivity)
    after = volume.commit()
    want += [volume.solidCount(), debris.solidCount(), after.n_nodes]
    rc = vrc.RayCaster(scene, (W, H))
    rc.setLightPosition(vrc.reference_light(depth))
    rc.use_gi = rc.use_samples = True
    rc.setScene(after)
    rc.renderFrame(vrc.reference_camera(depth, pitch=-0.5), spp=2)
    rc.samples_to_image()
    want.append(fnv1a(rc.readImage().tobytes()))
    print(out.stdout.strip())
    assert got == want

    seeds = np.zeros_like(dug)
    seeds[:, S // 2 + 1, :] = 1
    supported = flood_model.flood(dug, seeds, connectivity)
    air_seeds = np.zeros_like(dug)
    air_seeds[:, S - 1, :] = 1
    assert got[4] == int(supported.sum()) and got[5] == int(dug.sum()) - int(supported.sum()) >= 27
    assert got[2] == int(flood_model.flood(dug, air_seeds, connectivity, True).sum()) and got[3] == 1
    assert np.array_equal(volume.download(), supported)
