"""The sight methods through the C++ host adapter (HipVoxelDistance::sight / visibleFrom) against the model:
tests/cpp/voxel_sight_main.cpp prints FNV-1a hashes of its records and downloads, this file computes the same from
sight_model.py over the numpy distance field of the same world."""
import re

import numpy as np
import pytest

import distance_model
import sight_model as model
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_sight_matches_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_sight_main").stdout
    S = 16

    def value(name):
        return int(re.search(r"\b%s=(\d+)" % name, out).group(1))

    world = np.zeros((S, S, S), np.uint8)
    world[6:8, 0:12, 6:8] = 1
    world[0:16, 10:11, 0:5] = 1
    world[12, 3, 12] = 1
    D = distance_model.field(world)
    ends = [p for p in np.ndindex(S, S, S) if sum(p) % 3 == 0]
    segments = np.array([s + p for s in ((1, 1, 1), (15, 15, 15), (3, 14, 9), (7, 5, 7)) for p in ends] + [(1, 1, 1, S, 0, 0)], np.int32)
    assert value("segments") == len(segments)
    thin, touch = model.sight(D, S, segments, 1, model.NONE, False), model.sight(D, S, segments, 1, model.NONE, True)
    assert {int(s) for s in touch["status"]} == {model.CLEAR, model.BLOCKED, model.OUTSIDE} and thin.tobytes() != touch.tobytes()
    assert value("thin") == fnv1a(thin.tobytes())
    assert value("touch") == fnv1a(touch.tobytes()) == value("plain")
    assert value("ball") == fnv1a(model.sight(D, S, segments, 2, model.NONE, False).tobytes())
    assert value("band") == fnv1a(model.sight(D, S, segments, 4, 40, True).tobytes())

    eye = (3, 14, 9)
    seen = model.sight_field(D, eye, 0, 1, model.NONE, False)
    visible, max_d2, argmax = model.field_stats(seen)
    assert value("seen") == fnv1a(seen.tobytes()) and (value("visible"), value("max_d2")) == (visible, max_d2)
    assert re.search(r"argmax=%d,%d,%d connectivity=0\b" % argmax, out)
    near = model.sight_field(D, eye, 6, 1, model.NONE, True)
    assert value("near") == fnv1a(near.tobytes()) and value("near_visible") == int((near != model.NONE).sum()) < visible
    assert value("picked") == visible
