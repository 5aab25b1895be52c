"""The methods between depths through the C++ host adapter (HipVoxelVolume::cellCounts / reduceInto / reduced / expandInto /
expanded) against the numpy model: tests/cpp/voxel_levels_main.cpp prints FNV-1a hashes of its downloads and counts, this
file computes the same from levels_model.py."""
import re

import numpy as np
import pytest

import cells_model
import levels_model as model
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_levels_match_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_levels_main").stdout
    S = 32

    def value(name):
        return int(re.search(r"\b%s=(\d+)" % name, out).group(1))

    def digest(a, dtype=np.uint8):
        return fnv1a(np.ascontiguousarray(a, dtype).tobytes())

    world = cells_model.random_set(7, cells_model.threshold_of(0.5), S)
    assert value("filled") == digest(world)
    for k in range(1, 6):
        c = model.counts(world, k)
        assert (value("cells%d" % k), value("counts%d" % k), value("sum%d" % k)) == (c.size, digest(c, np.uint32), int(world.sum())), k
    assert (value("any4"), value("all4")) == (digest(model.reduced(world, 4, "any")), digest(model.reduced(world, 4, "all")))
    for depth in (4, 3, 2):
        assert value("half%d" % depth) == digest(model.reduced(world, depth, "majority")), depth

    coarse = cells_model.random_set(5, cells_model.threshold_of(0.5), 8)
    assert (value("lo"), value("hi")) == (32, 65) == model.count_range("majority", 2)
    band = model.reduce(coarse, world, 34, 65, model.ANDNOT)
    assert not np.array_equal(band, coarse) and band.any()
    assert value("band") == digest(band) and value("source") == digest(world)
    assert value("expanded") == digest(model.expand(np.zeros((64, 64, 64), np.uint8), band))
    assert value("merged") == digest(model.expand(world, band, model.OR))
    assert value("back") == digest(band)
