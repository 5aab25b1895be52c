"""The travel-distance field of the C++ host adapter (HipVoxelVolume::travelField, HipVoxelDistance::tracePaths /
connectivity / travelStats) compiled with plain g++ against the C ABI and run on the GPU at 16^3: a corridor with a side
room, a speck nothing reaches and a seed outside M.  Every number the program prints must be the breadth-first model's."""
import re

import numpy as np
import pytest

import travel_model as model
from volume_support import compile_cpp_main, run_program

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def program(built, tmp_path_factory):
    return compile_cpp_main(tmp_path_factory.mktemp("travel_cpp"), "voxel_travel_main")


@pytest.mark.parametrize("connectivity", [6, 26])
def test_cpp_travel_matches_the_model(program, connectivity):
    out = run_program(program, connectivity)

    S = 16
    vol = np.zeros((S, S, S), np.uint8)
    vol[1:14, 1:2, 1:2] = 1
    vol[13:14, 1:12, 1:2] = 1
    vol[5:8, 2:5, 1:3] = 1
    vol[13, 12, 1] = 1
    vol[2, 10, 10] = 1
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[1, 1, 1] = seeds[0, 0, 0] = 1
    T = model.field(vol, seeds, connectivity, False)
    n_seeds, reached, max_steps, argmax = model.stats(T, 1)

    m = re.search(r"seeds=(\d+) reached=(\d+) max_steps=(\d+) argmax=(\d+),(\d+),(\d+) sweeps=(\d+) reserved=(\d+) depth=(\d+) bytes=(\d+) connectivity=(\d+)",
                  out.stdout)
    assert m, out.stdout
    got = [int(g) for g in m.groups()]
    assert got[:6] + got[7:] == [n_seeds, reached, max_steps, *argmax, 0, 4, 4 * S ** 3, connectivity], out.stdout
    assert 1 <= got[6] <= 8 ** 4 + 1
    probes = [(1, 1, 1), (13, 12, 1), (7, 4, 2), (2, 10, 10)]
    m = re.search(r"at=(\d+),(\d+),(\d+),(\d+),(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [int(T[p]) for p in probes] + [model.NONE]
    assert int(T[2, 10, 10]) == model.NONE and int(T[13, 12, 1]) != model.NONE
    m = re.search(r"near=(\d+)", out.stdout)
    assert m and int(m.group(1)) == int(model.select(T, 0, 5).sum())
    m = re.search(r"lengths=(\d+),(\d+),(\d+)", out.stdout)
    assert m and [int(g) for g in m.groups()] == [int(T[13, 12, 1]), model.NONE, int(T[7, 4, 2])]
    length, route = model.trace(T, (13, 12, 1), connectivity)
    m = re.search(r"route=(\S*)", out.stdout)
    assert m and m.group(1) == "".join("%d,%d,%d;" % tuple(v) for v in route) and len(route) == length + 1 <= 32
    m = re.search(r"untouched=(\d+)", out.stdout)
    assert m and int(m.group(1)) == 32 * 3                     # the row of the start without a value keeps its fill
