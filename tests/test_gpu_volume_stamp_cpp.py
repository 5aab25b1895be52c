"""The affine stamp of the C++ host adapter (HipVoxelVolume::stampAffine / stampPlaced) compiled with plain g++ against the C
ABI and run on the GPU at 64^3: the two boxes, the voxel at the corner of one of them and the speck of the distance program,
turned a quarter turn and back, then placed with a 30-degree turn about two axes at scale 1.5 in a 128^3 world.  Every
solid count, every probe voxel and the placement's map the program prints must be the numpy model's."""
import re

import numpy as np
import pytest

import stamp_model as model
from volume_support import compile_cpp_main, run_program

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def program(built, tmp_path_factory):
    return compile_cpp_main(tmp_path_factory.mktemp("stamp_cpp"), "voxel_stamp_main")


def bits_at(vol, probes):
    return "".join(str(int(vol[tuple(p)])) for p in probes)


def test_cpp_stamp_matches_the_model(program):
    out = run_program(program)

    S = 64
    vol = np.zeros((S, S, S), np.uint8)
    vol[3:13, 4:10, 5:9] = 1
    vol[30:35, 30:33, 30:34] = 1
    vol[35, 33, 34] = 1
    vol[60, 1, 62] = 1
    probes = np.array([54, 12, 8, 58, 10, 6, 30, 35, 34, 62, 60, 62, 33, 28, 34, 1, 3, 62, 60, 1, 62, 0, 0, 0, 63, 63, 63, 32, 29, 33]).reshape(-1, 3)
    turn = model.signed_permutation((1, 0, 2), (0, 1, 0), S)
    back = model.signed_permutation((1, 0, 2), (1, 0, 0), S)
    turned = model.stamp(np.ones_like(vol), vol, *turn)
    restored = model.stamp(np.zeros_like(vol), turned, *back)
    assert np.array_equal(restored, vol) and not np.array_equal(turned, vol)
    m = re.search(r"solid=(\d+) turned=(\d+) restored=(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [int(vol.sum())] * 3
    assert re.search(r"turned_at=(\d+)", out.stdout).group(1) == bits_at(turned, probes)
    assert re.search(r"restored_at=(\d+)", out.stdout).group(1) == bits_at(vol, probes)
    assert "1" in bits_at(turned, probes) and "0" in bits_at(turned, probes)
    assert re.search(r"difference=(\d+)", out.stdout).group(1) == "0"

    rot = np.array([float(v) for v in re.search(r"rot=(\S+)", out.stdout).group(1).split(",")], np.float32)
    R = rot.astype(np.float64).reshape(3, 3).T
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.trace(R) - (2 * np.cos(np.radians(30)) + np.cos(np.radians(30)) ** 2)) < 1e-5
    want_m, want_t, lo, hi = model.place(rot, 1.5, (32.0,) * 3, (64.0,) * 3, 6, 7)
    m = re.search(r"map=([-\d,]+) reserved=(\d+) t=([-\d,]+)", out.stdout)
    assert m and [int(v) for v in m.group(1).split(",")] == want_m and m.group(2) == "0" and [int(v) for v in m.group(3).split(",")] == want_t
    world = np.zeros((128, 128, 128), np.uint8)
    world[60:68, 60:68, :] = 1
    placed = model.stamp(world, vol, want_m, want_t, lo, hi, model.OR)
    assert int(placed.sum()) > int(world.sum()) + int(vol.sum())            # scale 1.5: the paste adds more voxels than the model has
    assert int(re.search(r"world=(\d+)", out.stdout).group(1)) == int(placed.sum())
    far = np.array([64, 64, 64, 60, 60, 0, 49, 5, 36, 64, 66, 62, 51, 7, 40, 100, 64, 64, 64, 20, 64, 64, 64, 110, 40, 40, 40, 127, 127, 127]).reshape(-1, 3)
    assert re.search(r"world_at=(\d+)", out.stdout).group(1) == bits_at(placed, far)
