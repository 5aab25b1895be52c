"""The morphology methods through the C++ host adapter (HipVoxelVolume::morph / dilateBy / erodeBy / openBy / closeBy / fitsAt /
match and the element helpers) against the numpy model: tests/cpp/voxel_morph_main.cpp prints FNV-1a hashes of its downloads,
this file computes the same from morph_model.py."""
import re

import numpy as np
import pytest

import morph_model as model
from volume_support import fnv1a, run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_morph_matches_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_morph_main").stdout
    S = 32

    def value(name):
        return int(re.search(r"\b%s=(\d+)" % name, out).group(1))

    def digest(vol):
        return fnv1a(np.ascontiguousarray(vol, np.uint8).tobytes())

    def field(seed, density):
        return model.random_set(seed, model.threshold_of(density), S)

    world = field(7, 0.2)
    assert value("world") == digest(world) == value("source")
    held = model.apply(np.ones((S, S, S), np.uint8), world, model.DILATE, model.ball(3))
    assert value("ball") == digest(held)
    held = model.apply(held, world, model.ERODE, model.box(3, 5, 3, (0, 4, 1)), model.EMPTY, 0)
    assert 0 < held.sum() and value("box") == digest(held)
    held = model.apply(held, world, model.DILATE, model.cross(), model.SOLID, 1, model.OR)
    assert value("cross") == digest(held)
    held = model.apply(held, world, model.DILATE, model.reflect(model.line(2, 0, 16)), model.EMPTY, 0, model.ANDNOT)
    assert 0 < held.sum() and value("line") == digest(held)
    held = model.apply(held, world, model.ERODE, model.box(2, 3, 2) + np.array([9, 1, 30]), model.EMPTY, 1, model.REPLACE, (9, 1, 30))
    assert 0 < held.sum() < S ** 3 and value("origin") == digest(held)

    shape = model.morph(field(9, 0.5), model.DILATE, model.line(0, -2, 1))
    assert value("dilate_by") == digest(shape)
    shape = model.morph(shape, model.ERODE, model.box(2, 2, 2), outside=1)
    assert 0 < shape.sum() and value("erode_by") == digest(shape)
    shape = model.morph(shape, model.ERODE, model.cross(), outside=0)
    assert value("erode_open") == digest(shape)
    shape = field(13, 0.6)
    shape = model.morph(model.morph(shape, model.ERODE, model.ball(1), outside=1), model.DILATE, model.ball(1))
    assert 0 < shape.sum() and value("open_by") == digest(shape)
    shape = model.morph(model.morph(shape, model.DILATE, model.box(2, 1, 3)), model.ERODE, model.box(2, 1, 3), outside=1)
    assert value("close_by") == digest(shape)

    fits = model.fits_at(world, model.box(2, 3, 2))
    assert 0 < fits.sum() and value("fits") == digest(fits)
    solid_at, empty_at = [(0, 0, 0), (0, -1, 0)], [(1, 0, 0), (0, 0, 1)]
    found, walled = model.match(world, solid_at, empty_at), model.match(world, solid_at, empty_at, 1)
    assert 0 < found.sum() != walled.sum() > 0 and (value("match"), value("match_walled")) == (digest(found), digest(walled))
