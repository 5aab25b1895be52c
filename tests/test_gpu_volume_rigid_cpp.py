"""The rigid-piece mirrors of the C++ host adapter (HipVoxelLabels::moments / massProperties / poses / placeAffine) compiled
with plain g++ against the C ABI and run on the GPU at 16^3: two boxes, one with an arm, and a speck.  Every number the
program prints must be the numpy model's."""
import re

import numpy as np
import pytest

import components_model
import rigid_model as model
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_rigid_matches_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_rigid_main")

    S = 16
    debris = np.zeros((S, S, S), np.uint8)
    debris[1:7, 9:11, 1:6] = 1
    debris[9:12, 5:8, 9:15] = 1
    debris[10, 8:12, 9] = 1
    debris[3, 13, 3] = 1
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 3
    want = model.moments(ids, 3)

    m = re.search(r"count=(\d+)", out.stdout)
    assert m and int(m.group(1)) == 3
    got = [[int(v) for v in line.split(",")] for line in re.findall(r"moments=([\d,]+)", out.stdout)]
    assert got == [[n] + s1 + s2 for n, s1, s2 in want]
    assert re.search(r"window=2\n", out.stdout)
    props = re.findall(r"mass=(\S+) centre=(\S+),(\S+),(\S+) ixx=(\S+) ixy=(\S+)", out.stdout)
    assert len(props) == 3
    centres = []
    for line, case in zip(props, want):
        mass, centre, inertia = model.mass_properties(*case)
        values = [float(v) for v in line]
        assert values[0] == float(mass) and values[1:4] == [float(v) for v in centre]
        # the adapter divides once in long double: within one unit in the last place of the exact value
        for value, exact in ((values[4], inertia[0][0]), (values[5], inertia[0][1])):
            assert abs(value - float(exact)) <= abs(float(exact)) * 2.0 ** -52
        centres.append([float(v) for v in centre])
    quarter = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1], np.float32)
    maps, boxes = [], []
    for i in range(3):
        pivot = np.asarray(centres[i], np.float32)
        target = pivot + np.array([1, -2, 0], np.float32)
        mm, t, lo, hi = model.place_box(quarter, 1.0, pivot, target, rec["lo"][i], rec["hi"][i], 4)
        maps.append((mm, t))
        boxes.append(lo + hi)
    lines = re.findall(r"map=([-\d,]+) t=([-\d,]+) box=([\d,]+)", out.stdout)
    assert [([int(v) for v in a.split(",")], [int(v) for v in b.split(",")], [int(v) for v in c.split(",")]) for a, b, c in lines] == \
        [(mm, t, box) for (mm, t), box in zip(maps, boxes)]
    placed = model.place_affine(ids, maps, boxes, np.zeros((S, S, S), np.uint8))
    m = re.search(r"placed=(\d+)", out.stdout)
    assert m and int(m.group(1)) == int(placed.sum()) > 0
    m = re.search(r"without_first=(\d+)", out.stdout)
    assert m and int(m.group(1)) == int(model.place_affine(ids, maps, None, placed, model.ANDNOT, [1, 0, 0]).sum()) < int(placed.sum())
