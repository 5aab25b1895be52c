"""The contact mirror of the C++ host adapter (HipVoxelLabels::contacts) compiled with plain g++ against the C ABI and run on
the GPU at 16^3: the three pieces of the rigid C++ test over a slab.  Every record the program prints must be the numpy
model's."""
import re

import numpy as np
import pytest

import components_model
import contact_model as model
import rigid_model
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_contacts_match_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_contacts_main")

    S = 16
    debris = np.zeros((S, S, S), np.uint8)
    debris[1:7, 9:11, 1:6] = 1
    debris[9:12, 5:8, 9:15] = 1
    debris[10, 8:12, 9] = 1
    debris[3, 13, 3] = 1
    world = np.zeros((S, S, S), np.uint8)
    world[:, 0:2, :] = 1
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 3
    maps = rigid_model.translation_maps([[0, -7, 0], [0, 0, 0], [0, -4, 0]])

    def printed(tag):
        rows = [[int(v) for v in line.split(",")] for line in re.findall(r"^%s=([-\d,]+)$" % tag, out.stdout, re.M)]
        assert all(len(r) == 16 and r[15] == 0 for r in rows)
        return [(r[0], r[1], r[2:5], r[5:8], r[8], r[9:12], r[12:15]) for r in rows]

    m = re.search(r"count=(\d+)", out.stdout)
    assert m and int(m.group(1)) == 3
    want = model.contacts(ids, maps, None, world)
    assert want[0][1] == 0 and want[0][4] == 30 and want[1][1:] == model.ZERO[1:] and want[2][1] == 18     # rests, floats, sinks in
    assert printed("contact") == want
    boxes = [[0, 0, 0, 4, 16, 16], [0, 0, 0, 16, 16, 16], [0, 0, 0, 16, 16, 16]]
    kept = model.contacts(ids, maps, boxes, world, [1, 1, 0])
    assert kept[0][0] == 30 and kept[2] == model.ZERO
    assert printed("kept") == kept
