"""The deltas through the C++ host adapter (HipVoxelDelta, HipVoxelVolume::diff / applyDelta, HipVoxelHistory) against the numpy
model: tests/cpp/voxel_delta_main.cpp prints FNV-1a hashes of its downloads and records, this file computes the same from
delta_model.py."""
import re

import numpy as np
import pytest

import delta_model as model
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_deltas_match_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_delta_main").stdout
    S, depth = 64, 6
    before = np.zeros((S, S, S), np.uint8)
    before[:, :30, :] = 1
    before[20:41, 30:37, 20:45] = 1
    x, y, z = np.ogrid[:S, :S, :S]
    after = before.copy()
    after[(x - 31) ** 2 + (y - 29) ** 2 + (z - 33) ** 2 <= 81] = 0
    records, stats = model.diff(model.words_of(before), model.words_of(after), depth)
    assert stats["words"] > 8

    def value(name):
        return int(re.search(r"\b%s=(\d+)" % name, out).group(1))

    assert value("before") == fnv1a(before.tobytes()) and value("after") == fnv1a(after.tobytes())
    m = re.search(r"stats words=(\d+) voxels=(\d+) lo=(\d+),(\d+),(\d+) hi=(\d+),(\d+),(\d+) reserved=(\d+),(\d+)", out)
    got = [int(g) for g in m.groups()]
    assert (got[0], got[1], tuple(got[2:5]), tuple(got[5:8]), tuple(got[8:])) == model.stats_tuple(stats)
    assert [value(k) for k in ("count", "depth", "bytes", "records")] == [len(records), depth, 8 * len(records), fnv1a(records.tobytes())]
    assert "window=5 same" in out
    assert value("applied") == fnv1a(after.tobytes()) and value("again") == fnv1a(before.tobytes())
    assert value("copy") == fnv1a(after.tobytes()) and len(re.findall(r"voxels=%d\b" % stats["voxels"], out)) == 2

    built_on = after.copy()
    built_on[5:9, 40:44, 5:9] = 1
    step, _ = model.diff(model.words_of(after), model.words_of(built_on), depth)
    assert value("idle") == 0 and value("step") == 64 and value("built") == fnv1a(built_on.tobytes())
    assert value("undo") == len(step) and value("undone") == fnv1a(after.tobytes())
    assert value("redo") == len(step) and value("redone") == fnv1a(built_on.tobytes())
    assert re.findall(r"stacks=(\d+),(\d+)", out) == [("0", "1"), ("1", "0")]
    assert re.search(r"stacks=1,0 bytes=(\d+)", out).group(1) == str(8 * len(step)) and value("nothing") == 0
