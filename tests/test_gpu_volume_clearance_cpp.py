"""The clearance mirror of the C++ host adapter (HipVoxelLabels::clearance) compiled with plain g++ against the C ABI and run on
the GPU at 32^3: four loose pieces, each moved by an offset of its own, over the distance to a world's solid and over a travel
field through its air.  The program prints the FNV-1a checksum of the records' bytes; it must be the checksum of the Python
call's records, which must be the numpy model's."""
import re

import numpy as np
import pytest

import clearance_model as model
import components_model
import distance_model
import rigid_model
import travel_model
from volume_support import affine_records, fnv1a, labels_of, run_cpp_main, volume_of

pytestmark = pytest.mark.gpu


def test_cpp_clearance_matches_python_and_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_clearance_main")

    S = 32
    lo_hi = np.array([[2, 20, 2, 8, 23, 9], [12, 18, 12, 15, 26, 14], [20, 22, 5, 29, 24, 8], [25, 28, 25, 26, 29, 26]])
    debris = np.zeros((S, S, S), np.uint8)
    for b in lo_hi:
        debris[b[0]:b[3], b[1]:b[4], b[2]:b[5]] = 1
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 4 and np.array_equal(np.concatenate([rec["lo"], rec["hi"]], 1), lo_hi)
    world = np.zeros((S, S, S), np.uint8)
    world[:, 0:3, :] = 1
    world[14:18, 3:20, 14:18] = 1
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[0, 31, 0] = 1
    offsets = np.array([[3, -12, 1], [2, -6, 3], [-4, -19, 6], [-20, -3, 1]])
    maps = rigid_model.translation_maps(offsets)
    boxes = rigid_model.moved_boxes(rec, offsets, S)
    boxes[2, 4] -= 1
    keep = np.array([1, 0, 1, 1], np.uint8)

    m = re.search(r"count=(\d+)", out.stdout)
    assert m and int(m.group(1)) == 4
    printed = {tag: int(value) for tag, value in re.findall(r"^(solid|boxed|kept)=(\d+)$", out.stdout, re.M)}

    labels, volume, seed_volume = labels_of(debris, 6), volume_of(world), volume_of(seeds)
    solid, travel = volume.distanceField(False, False), volume.travelField(seed_volume, 6, True)
    D, T = distance_model.field(world), travel_model.field(world, seeds, 6, True)
    records = affine_records(maps)
    cases = {"solid": (solid, D, None, None), "boxed": (solid, D, boxes, None), "kept": (travel, T, boxes, keep)}
    for tag, (field, dense, bx, kp) in cases.items():
        got = labels.clearance(records, field, bx, kp)
        assert model.tuples(got) == model.clearance(ids, maps, bx, dense, kp), tag
        assert printed[tag] == fnv1a(got.tobytes()), tag
    whole = model.clearance(ids, maps, None, D)
    assert whole[1][3] == 0 and whole[2][3] == 1 and whole[0][3] > 1           # one piece inside the pillar, one resting on the floor, one clear
    assert model.clearance(ids, maps, boxes, D)[2] != whole[2]                # the cut box shows
    for v in (solid, travel, labels, volume, seed_volume):
        v.close()
