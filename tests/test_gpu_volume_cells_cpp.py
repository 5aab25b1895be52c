"""The cell methods through the C++ host adapter (HipVoxelVolume::cellStep / automaton / smooth / removeSpecks / fillRandom /
caves) against the numpy model: tests/cpp/voxel_cells_main.cpp prints FNV-1a hashes of its downloads, this file computes the
same from cells_model.py."""
import re

import numpy as np
import pytest

import cells_model as model
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_cells_match_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_cells_main").stdout
    S = 32

    def value(name):
        return int(re.search(r"\b%s=(\d+)" % name, out).group(1))

    def digest(vol):
        return fnv1a(np.ascontiguousarray(vol, np.uint8).tobytes())

    world = model.fill_random(np.zeros((S, S, S), np.uint8), 7, model.threshold_of(0.45))
    assert value("filled") == digest(world)
    world = model.fill_random(world, 11, model.threshold_of(0.5), (3, 5, 7, 30, 21, 18), model.ANDNOT)
    assert value("boxed") == digest(world)

    nxt, changed = model.step(world, 0x1E0, 0x7FF0, 26, 1)
    assert changed > 0 and (value("all"), value("changed_all")) == (digest(nxt), changed)
    nxt, changed = model.step(world, 1 << 3, 0x7C, 6, 0)
    assert changed > 0 and (value("faces"), value("changed_faces")) == (digest(nxt), changed)
    assert value("source") == digest(world) and value("async") == digest(nxt)

    state, taken = model.automaton(world, 3, model.SMOOTH_BIRTH, model.SMOOTH_SURVIVE, 26, 0)
    assert taken == 3 and (value("taken"), value("automaton")) == (3, digest(state))
    state, more = model.automaton(state, 100, model.SMOOTH_BIRTH, model.SMOOTH_SURVIVE, 26, 0)
    assert 0 < more < 100 and (value("to_fixed"), value("fixed")) == (more, digest(state))

    dust = model.fill_random(np.zeros((S, S, S), np.uint8), 3, model.threshold_of(0.1))
    cleaned = model.remove_specks(dust)
    assert 0 < cleaned.sum() < dust.sum() and value("specks") == digest(cleaned)
    dust = model.smooth(model.random_set(5, model.threshold_of(0.5), S), 2, 1)
    assert value("smooth") == digest(dust)
    assert value("caves") == digest(model.caves(S, 1337, 0.48, 4))
