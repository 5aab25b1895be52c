"""The pair-contact mirror of the C++ host adapter (HipVoxelLabels::candidatePairs / pairContacts) compiled with plain g++
against the C ABI and run on the GPU at 16^3: the three pieces of the rigid C++ test, moved onto and next to each other.  The
pairs and every record the program prints must be the numpy model's."""
import re

import numpy as np
import pytest

import components_model
import pair_contact_model as model
import rigid_model
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_pair_contacts_match_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_pair_contacts_main")

    S = 16
    debris = np.zeros((S, S, S), np.uint8)
    debris[1:7, 9:11, 1:6] = 1
    debris[9:12, 5:8, 9:15] = 1
    debris[10, 8:12, 9] = 1
    debris[3, 13, 3] = 1
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 3
    offsets = np.array([[6, 2, 7], [3, -2, 6], [0, 0, 0]])
    maps = rigid_model.translation_maps(offsets)
    boxes = rigid_model.moved_boxes(rec, offsets, S)

    def printed(tag):
        rows = [[int(v) for v in line.split(",")] for line in re.findall(r"^%s=([-\d,]+)$" % tag, out.stdout, re.M)]
        assert all(len(r) == 16 and r[15] == 0 for r in rows)
        return [(r[0], r[1], r[2:5], r[5:8], r[8], r[9:12], r[12:15]) for r in rows]

    def printed_pairs(tag):
        return [tuple(int(v) for v in line.split(",")) for line in re.findall(r"^%s=([\d,]+)$" % tag, out.stdout, re.M)]

    m = re.search(r"count=(\d+)", out.stdout)
    assert m and int(m.group(1)) == 3
    pairs = model.box_pairs(boxes, S)
    assert printed_pairs("pair") == [tuple(p) for p in pairs.tolist()] and len(pairs) >= 4
    want = model.pair_contacts(ids, maps, boxes, pairs, S)
    assert sum(w[1] > 0 for w in want) >= 2 and sum(w[4] > 0 for w in want) >= 2          # the boxes sink in, the speck touches
    assert printed("contact") == want
    keep = [1, 0, 1]
    assert printed_pairs("keptpair") == [tuple(p) for p in model.box_pairs(boxes, S, keep).tolist()]
    kept = model.pair_contacts(ids, maps, None, [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0)], S, keep)
    assert kept[1][0] > 0 and kept[1][1:] == model.ZERO[1:] and kept[3] == model.ZERO
    assert printed("kept") == kept
