"""The distance field of the C++ host adapter (HipVoxelDistance, HipVoxelVolume::distanceField / dilate / erode / hollow)
compiled with plain g++ against the C ABI and run on the GPU at 64^3: the two boxes, the voxel at the corner of one of them
and the speck of the components program.  Every number the program prints must be the numpy model's."""
import re

import numpy as np
import pytest

import distance_model as model
from volume_support import compile_cpp_main, run_program

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def program(built, tmp_path_factory):
    return compile_cpp_main(tmp_path_factory.mktemp("distance_cpp"), "voxel_distance_main")


@pytest.mark.parametrize("to_empty,outside", [(False, False), (True, True)])
def test_cpp_distance_matches_the_model(program, to_empty, outside):
    out = run_program(program, int(to_empty), int(outside))

    S = 64
    vol = np.zeros((S, S, S), np.uint8)
    vol[3:13, 4:10, 5:9] = 1
    vol[30:35, 30:33, 30:34] = 1
    vol[35, 33, 34] = 1
    vol[60, 1, 62] = 1
    D = model.field(vol, to_empty, outside)
    max_d2, argmax = model.stats(D)
    features = int(model.feature_set(vol, to_empty).sum())

    m = re.search(r"features=(\d+) max_d2=(\d+) argmax=(\d+),(\d+),(\d+) reserved=(\d+) depth=(\d+) bytes=(\d+) data=(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [features, max_d2, *argmax, 0, 6, 4 * S ** 3, 1], out.stdout
    probes = [(3, 4, 5), (34, 32, 33), (0, 0, 0), (63, 63, 0)]
    m = re.search(r"at=(\d+),(\d+),(\d+),(\d+),(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [int(D[p]) for p in probes] + [model.NONE]
    m = re.search(r"voxels=(\d+) sum=(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [S ** 3, int(D[D != model.NONE].sum(dtype=np.uint64))]
    m = re.search(r"shell=(\d+)", out.stdout)
    assert m and int(m.group(1)) == int(model.select(D, 1, 4).sum())
    grown = model.dilate(vol, 2).astype(np.uint8)
    shrunk = model.erode(grown, 2, outside).astype(np.uint8)
    shell = model.hollow(shrunk, 1)
    m = re.search(r"before=(\d+) dilate=(\d+) erode=(\d+) hollow=(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [int(vol.sum()), int(grown.sum()), int(shrunk.sum()), int(shell.sum())]
