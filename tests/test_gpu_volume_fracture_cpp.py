"""The fracture mirror of the C++ host adapter (HipVoxelVolume::fracture, HipVoxelLabels::pieceSites) compiled with plain g++
against the C ABI and run on the GPU at 64^3: a wall on a slab broken round five sites.  Every record and every piece's cell
the program prints must be the numpy model's."""
import re

import numpy as np
import pytest

import fracture_model as model
from volume_support import run_cpp_main

pytestmark = pytest.mark.gpu


def test_cpp_fracture_matches_the_model(built, tmp_path):
    out = run_cpp_main(tmp_path, "voxel_fracture_main")

    S = 64
    world = np.zeros((S, S, S), np.uint8)
    world[:, 0:3, :] = 1
    world[10:54, 3:40, 28:33] = 1
    sites = [[30, 20, 30], [36, 25, 31], [-4, 20, 30], [30, 20, 30], [33, 14, 29]]
    for tag, connectivity, max_d2 in (("near", 6, 144), ("all", 26, model.NONE)):
        ids, rec, ps = model.label(world, sites, connectivity, False, max_d2)
        want = [r["first"].tolist() + r["lo"].tolist() + r["hi"].tolist() + [0, int(r["voxels"]), int(c)] for r, c in zip(rec, ps)]
        rows = [[int(v) for v in line.split(",")] for line in re.findall(r"^%s=([\d,]+)$" % tag, out.stdout, re.M)]
        assert rows == want, tag
        assert re.search(r"^%s_count=%d,%d$" % (tag, len(rec), 4 * S ** 3 + 52 * len(rec)), out.stdout, re.M), out.stdout[:300]
        assert re.search(r"^%s_window=%d$" % (tag, max(0, min(2, len(rec) - 1))), out.stdout, re.M)
        cells = sorted(set(ps.tolist()))
        assert cells == ([0, 1, 4, model.NONE] if tag == "near" else [0, 1, 4]), cells          # the duplicate and the outside site own nothing
        print(f"{tag}: {len(rec)} pieces, cells {cells}")
