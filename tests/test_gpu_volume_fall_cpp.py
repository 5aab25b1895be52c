"""The falling pieces of the C++ host adapter (HipVoxelLabels::fall / place, HipVoxelVolume::dropLoose) compiled with plain
g++ against the C ABI and run on the GPU at 16^3: a slab with a ledge, three loose boxes and a speck.  Every number the
program prints must be the numpy model's."""
import re

import numpy as np
import pytest

import components_model
import fall_model as model
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu
DOWN = 2                                               # VRC_FACE_YN


@pytest.mark.parametrize("connectivity,limit", [(6, 0), (26, 3)])
def test_cpp_fall_matches_the_model(built, tmp_path, connectivity, limit):
    out = run_cpp_main(tmp_path, "voxel_fall_main", connectivity, limit)

    S = 16
    fixed = np.zeros((S, S, S), np.uint8)
    fixed[:, 0:2, :] = 1
    fixed[2:5, 2:6, 2:5] = 1
    debris = np.zeros((S, S, S), np.uint8)
    debris[1:7, 9:11, 1:7] = 1
    debris[3:5, 13, 3:5] = 1
    debris[9:12, 5:8, 9:15] = 1
    debris[10, 12, 10] = 1
    ids, rec = components_model.label(debris, connectivity)
    assert len(rec) == 4
    D = model.drops(ids, fixed, DOWN, limit)
    want = model.offsets_of(D, DOWN)
    assert (D > 0).all() and (limit or sorted(D.tolist()) == [3, 3, 5, 7])

    m = re.search(r"count=(\d+)", out.stdout)
    assert m and int(m.group(1)) == len(rec)
    got = [tuple(int(v) for v in g) for g in re.findall(r"offset=(-?\d+),(-?\d+),(-?\d+)", out.stdout)]
    assert got == [tuple(int(v) for v in row) for row in want]
    m = re.search(r"stats moved_voxels=(\d+) pieces=(\d+) moved_pieces=(\d+) max_drop=(\d+) reserved=0,0", out.stdout)
    assert m and tuple(int(g) for g in m.groups()) == model.stats(ids, D)
    m = re.search(r"rounds=(\d+)", out.stdout)
    assert m and 1 <= int(m.group(1)) <= len(rec) + 1
    placed = model.place(ids, want, fixed)
    m = re.search(r"placed=(\d+)", out.stdout)
    assert m and int(m.group(1)) == int(placed.sum()) == int(fixed.sum()) + int(debris.sum())
    keep = np.zeros(len(rec), np.uint8)
    keep[0] = 1
    m = re.search(r"without_first=(\d+)", out.stdout)
    assert m and int(m.group(1)) == int(model.place(ids, want, placed, False, keep).sum())
    # dropLoose on the world itself: the anchor is the slab's bottom layer, the ledge holds on to it, the rest is the debris
    m = re.search(r"dropped moved_voxels=(\d+) pieces=(\d+) moved_pieces=(\d+) max_drop=(\d+) before=(\d+) after=(\d+)", out.stdout)
    total = int(fixed.sum()) + int(debris.sum())
    assert m and tuple(int(g) for g in m.groups()) == model.stats(ids, D) + (total, total)
