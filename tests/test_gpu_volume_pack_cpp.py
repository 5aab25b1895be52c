"""The sparse tile stream through the C++ host adapter (HipVoxelVolume::packInfo / pack / unpack / save / load):
tests/cpp/volume_pack_main.cpp saves a volume to a file and loads it into a second one; the downloads are equal, and the
file's bytes are the numpy model's and Python's pack() of the same field."""
import re

import numpy as np
import pytest

import pack_model as model
from volume_support import fnv1a, run_cpp_main, volume_of

pytestmark = pytest.mark.gpu


def test_cpp_save_and_load(built, tmp_path):
    path = tmp_path / "world.vrcp"
    out = run_cpp_main(tmp_path, "volume_pack_main", path).stdout
    S, depth = 64, 6
    field = np.zeros((S, S, S), np.uint8)
    field[:, :30, :] = 1
    field[20:41, 30:37, 20:45] = 1
    x, y, z = np.ogrid[:S, :S, :S]
    field[(x - 31) ** 2 + (y - 29) ** 2 + (z - 33) ** 2 <= 81] = 0
    want = model.pack(field, depth)
    h = model.header_of(want)

    def value(name):
        return int(re.search(r"\b%s=(\d+)" % name, out).group(1))

    assert value("saved") == value("loaded") == value("kept") == fnv1a(field.tobytes())
    m = re.search(r"info depth=(\d+) tiles=(\d+) mixed=(\d+) full=(\d+) partial=(\d+) bytes=(\d+) solid=(\d+)", out)
    assert [int(g) for g in m.groups()] == [depth, h[3], h[4], h[10], h[5], len(want), int(field.sum())]
    assert value("depth") == depth and value("count") == int(field.sum())
    assert path.read_bytes() == want
    assert value("stream") == fnv1a(want) and value("size") == len(want)
    assert re.search(r"refused=.*vrc_unpack_volume: rule solid-count", out), out
    volume = volume_of(field, depth)
    assert volume.pack().tobytes() == want
    volume.close()
