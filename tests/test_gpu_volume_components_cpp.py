"""The connected components of the C++ host adapter (HipVoxelLabels, HipVoxelVolume::labelComponents / removeSmallPieces)
compiled with plain g++ against the C ABI and run on the GPU at 64^3: two boxes, a voxel at the corner of one of them and
a speck.  Every number the program prints must be the numpy model's."""
import re

import numpy as np
import pytest

import components_model as model
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("connectivity", [6, 26])
def test_cpp_components_match_the_model(built, tmp_path, connectivity):
    out = run_cpp_main(tmp_path, "voxel_components_main", connectivity)

    S = 64
    vol = np.zeros((S, S, S), np.uint8)
    vol[3:13, 4:10, 5:9] = 1
    vol[30:35, 30:33, 30:34] = 1
    vol[35, 33, 34] = 1
    vol[60, 1, 62] = 1
    ids, rec = model.label(vol, connectivity)
    assert len(rec) == (4 if connectivity == 6 else 3)

    m = re.search(r"count=(\d+) depth=(\d+) bytes=(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [len(rec), 6, 4 * S ** 3 + 48 * len(rec)], out.stdout
    got = re.findall(r"record first=(\d+),(\d+),(\d+) lo=(\d+),(\d+),(\d+) hi=(\d+),(\d+),(\d+) reserved=(\d+) voxels=(\d+)", out.stdout)
    want = [tuple(str(int(v)) for v in (*r["first"], *r["lo"], *r["hi"], r["reserved"], r["voxels"])) for r in rec]
    assert got == want
    probes = [(3, 4, 5), (34, 32, 33), (35, 33, 34), (60, 1, 62), (0, 0, 0)]
    m = re.search(r"at=(\d+),(\d+),(\d+),(\d+),(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [int(ids[p]) for p in probes]
    assert int(ids[0, 0, 0]) == model.NO_COMPONENT
    m = re.search(r"window=1 first=(\d+),(\d+),(\d+)", out.stdout)
    assert m and tuple(int(g) for g in m.groups()) == tuple(int(v) for v in rec[1]["first"])
    m = re.search(r"piece=(\d+)", out.stdout)
    assert m and int(m.group(1)) == int(rec[1]["voxels"]) == (60 if connectivity == 6 else 61)
    kept = model.despeckle(vol, 2, connectivity)
    m = re.search(r"before=(\d+) removed=(\d+) after=(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [int(vol.sum()), int((rec["voxels"] < 2).sum()), int(kept.sum())]
    m = re.search(r"again=(\d+) snapshot=(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [len(model.label(kept, connectivity)[1]), len(rec)]
