"""The column methods through the C++ host adapter (HipVoxelVolume::columnProfile / heightMap / thicknessMap / isHeightField /
fillColumns / raiseTerrain / selectColumns / skyLit / topLayers / sheltered) against the numpy model:
tests/cpp/voxel_columns_main.cpp prints FNV-1a hashes of its records and downloads, this file computes the same from
columns_model.py.  Its last lines are the record of one comb column of 512^3 (256 runs), expected from columns_cases.py."""
import re

import numpy as np
import pytest

import cells_model
import columns_cases
import columns_model as model
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_columns_match_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_columns_main").stdout
    S = 32

    def value(name):
        return int(re.search(r"\b%s=(-?\d+)" % name, out).group(1))

    def digest(a, dtype=np.uint8):
        return fnv1a(np.ascontiguousarray(a, dtype).tobytes())

    world = cells_model.fill_random(np.zeros((S, S, S), np.uint8), 7, cells_model.threshold_of(0.45))
    for d in model.DIRECTIONS:
        assert value("profile%d" % d) == digest(model.profile(world, d), model.COLUMN_DTYPE), d
    rect = (3, 5, 30, 18)
    assert value("rect") == digest(model.profile(world, 2, rect), model.COLUMN_DTYPE)
    assert value("height") == digest(model.height_map(world, 2, -7), np.int32)
    assert value("thickness") == digest(model.thickness_map(world, 0), np.uint32)
    assert not model.is_height_field(world, 2) and re.search(r"thickness=\d+ field=0", out)

    u, v = np.meshgrid(np.arange(3, 30), np.arange(5, 18), indexing="ij")
    lo, hi = u - 3, 2 * v - 9
    world = model.fill(world, 0, lo, hi, rect, model.REPLACE)
    assert value("replace") == digest(world)
    world = model.fill(world, 2, 4, hi, rect, model.OR)
    assert value("or") == digest(world)
    world = model.fill(world, 1, lo, 20, rect, model.ANDNOT)
    assert value("andnot") == digest(world)
    world = model.fill(world, 1, 30, 31)
    assert value("slab") == digest(world)

    x, z = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    other = model.raise_terrain((x * 7 + z * 5) % 41 - 4, 5)
    assert value("terrain") == digest(other)
    assert model.is_height_field(other, 2) and not model.is_height_field(other, 2, grounded=True)
    assert re.search(r"terrain=\d+ field=1 grounded=0", out)

    other = model.select(other, world, 5, 2, 6, model.BOTH, model.OR)
    assert value("select") == digest(other) and value("source") == digest(world)
    assert value("lit") == digest(model.selection(world, 2, 0, 1, model.SOLID))
    assert value("top") == digest(model.selection(world, 1, 0, 3, model.SOLID))
    assert value("sheltered") == digest(model.selection(world, 4, 1, S + 1, model.EMPTY))

    comb = tuple((y, y + 1) for y in range(1, 512, 2))
    assert comb in [runs for _, runs in columns_cases.catalogue(512)]            # "comb 256 from 1"
    for side in (0, 1):
        want = columns_cases.record_tuple(comb, 512, side)
        assert want == ((1, 511, 256, 256) if side else (511, 1, 256, 256))
        assert re.search(r"\bcomb%d=%d,%d,%d,%d size=1\b" % ((side,) + want), out), (side, want)
    assert value("comb_solid") == 256
