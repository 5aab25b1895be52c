"""Voronoi fracture on a machine without a GPU: the yardstick of the GPU tests itself -- tests/fracture_model.py against a
literal per-voxel, per-site loop and against a breadth-first search --, its reduction to the plain labelling, the refusals
that need no device, scatter_sites, and the C++ host adapter under a plain C++14 compiler."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest

import components_model
import fracture_model as model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = model.NONE


def cells_literally(S, sites, max_d2):
    """the rule as written: for every voxel, every site in index order, a strictly smaller distance replaces the choice"""
    out = np.full((S, S, S), NONE, np.uint32)
    for x in range(S):
        for y in range(S):
            for z in range(S):
                best, arg = None, NONE
                for i, (sx, sy, sz) in enumerate(sites):
                    if not (0 <= sx < S and 0 <= sy < S and 0 <= sz < S):
                        continue
                    d2 = (x - sx) ** 2 + (y - sy) ** 2 + (z - sz) ** 2
                    if best is None or d2 < best:
                        best, arg = d2, i
                if best is not None and (max_d2 == NONE or best <= max_d2):
                    out[x, y, z] = arg
    return out


def pieces_by_search(M, cell, connectivity):
    """breadth-first search from every voxel of M in key order: ids by ascending key of the first voxel met"""
    S = M.shape[0]
    K = components_model.keys(S)
    ids = np.full((S, S, S), NONE, np.uint32)
    order = sorted((int(K[tuple(v)]), tuple(v)) for v in np.argwhere(M).tolist())
    offsets = model.offsets_of(connectivity)
    count = 0
    for _, v in order:
        if ids[v] != NONE:
            continue
        ids[v] = count
        todo = deque([v])
        while todo:
            p = todo.popleft()
            for d in offsets:
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if min(q) < 0 or max(q) >= S or not M[q] or ids[q] != NONE or cell[q] != cell[p]:
                    continue
                ids[q] = count
                todo.append(q)
        count += 1
    return ids


def random_sites(rng, S, n):
    """n sites, some outside the volume and some duplicated"""
    sites = rng.integers(-2, S + 2, (n, 3))
    if n > 2:
        sites[n // 2] = sites[0]
    return sites.astype(np.int32)


@pytest.mark.parametrize("S", [4, 8])
def test_cells_against_the_literal_loop(S):
    rng = np.random.default_rng(900 + S)
    for n in (1, 2, 7, 40):
        for max_d2 in (NONE, 0, 2, 9):
            sites = random_sites(rng, S, n)
            assert np.array_equal(model.cells(S, sites, max_d2), cells_literally(S, sites.tolist(), max_d2)), (S, n, max_d2)
    # ties: two sites an even distance apart, in both orders -- the middle plane goes to the lower index
    for order in ((0, 1), (1, 0)):
        sites = np.array([[0, 1, 1], [2, 1, 1]])[list(order)]
        cell = model.cells(S, sites)
        assert (cell[1] == 0).all() and np.array_equal(cell, cells_literally(S, sites.tolist(), NONE))


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("S", [4, 8])
def test_label_against_a_search(S, connectivity):
    rng = np.random.default_rng(950 + S + connectivity)
    for trial in range(6):
        medium = (rng.random((S, S, S)) < (0.6, 0.9, 0.3)[trial % 3]).astype(np.uint8)
        sites = random_sites(rng, S, (1, 3, 9)[trial % 3])
        max_d2 = (NONE, 4)[trial % 2]
        for through_empty in (False, True):
            ids, rec, ps = model.label(medium, sites, connectivity, through_empty, max_d2)
            M = (medium == 0) if through_empty else (medium != 0)
            cell = model.cells(S, sites, max_d2)
            assert np.array_equal(ids, pieces_by_search(M, cell, connectivity)), (S, connectivity, trial, through_empty)
            assert int(rec["voxels"].sum()) == int(M.sum()) and len(ps) == len(rec)
            for i in range(len(rec)):
                assert (cell[ids == i] == ps[i]).all()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_no_site_in_the_volume_is_the_plain_labelling(connectivity):
    S = 8
    rng = np.random.default_rng(77 + connectivity)
    medium = (rng.random((S, S, S)) < 0.35).astype(np.uint8)
    want_ids, want_rec = components_model.label(medium, connectivity)
    outside = np.array([[-1, 0, 0], [S, 3, 3], [2, 2, 1 << 20]])
    ids, rec, ps = model.label(medium, outside, connectivity)
    assert np.array_equal(ids, want_ids) and rec.tobytes() == want_rec.tobytes() and (ps == NONE).all()
    # and so is a cut-off below every distance: sites on empty voxels, max_d2 = 0
    empty = np.argwhere(medium == 0)[:5]
    ids, rec, ps = model.label(medium, empty, connectivity, False, 0)
    assert np.array_equal(ids, want_ids) and rec.tobytes() == want_rec.tobytes() and (ps == NONE).all()


def test_scatter_sites():
    from cpuvoxelraycaster_amd import scenes
    a = scenes.scatter_sites((40, 50, 60), 9, 200, 5)
    b = scenes.scatter_sites((40, 50, 60), 9, 200, 5)
    assert a.dtype == np.int32 and a.shape == (200, 3) and np.array_equal(a, b)
    d = a.astype(np.int64) - (40, 50, 60)
    assert ((d * d).sum(axis=1) <= 81).all()
    assert ((d * d).sum(axis=1) > 36).any() and len(np.unique(a, axis=0)) > 150          # it fills the ball
    assert not np.array_equal(a, scenes.scatter_sites((40, 50, 60), 9, 200, 6))
    assert scenes.scatter_sites((1, 2, 3), 0, 4, 0).tolist() == [[1, 2, 3]] * 4
    assert scenes.scatter_sites((1, 2, 3), 5, 0, 0).shape == (0, 3)
    with pytest.raises(ValueError):
        scenes.scatter_sites((0, 0, 0), -1, 3, 0)


def test_fracture_refusals_need_no_gpu(built):
    """NULL medium / out, no sites, NULL sites, 2^32 - 1 sites and more, a bad connectivity, through or mem are
    VRC_ERR_INVALID with the function's name before any HIP call: the handles here are not volumes or labels at all, and
    nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, c = (C.c_uint32 * 128)(), (C.c_uint32 * 128)()
    pa, pc = C.cast(a, C.c_void_p), C.cast(c, C.c_void_p)
    sites = np.zeros((4, 3), np.int32)
    out, count = C.c_void_p(0x1234), C.c_uint64(99)
    H, D = capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE

    def refused(text, *args):
        assert L.vrc_fracture_label(*args) == -1
        assert L.vrc_last_error().startswith(b"vrc_fracture_label: " + text), L.vrc_last_error()

    for mem in (H, D):
        refused(b"null argument", None, 6, 0, 4, capi.ptr(sites), NONE, mem, C.byref(out), C.byref(count))
        refused(b"null argument", pa, 6, 0, 4, capi.ptr(sites), NONE, mem, None, C.byref(count))
        for connectivity in (0, 7, 18, -6):
            refused(b"connectivity", pa, connectivity, 0, 4, capi.ptr(sites), NONE, mem, C.byref(out), C.byref(count))
        for through in (-1, 2):
            refused(b"bad through", pa, 26, through, 4, capi.ptr(sites), NONE, mem, C.byref(out), C.byref(count))
        refused(b"no sites", pa, 6, 1, 0, capi.ptr(sites), NONE, mem, C.byref(out), C.byref(count))
        refused(b"no sites", pa, 6, 1, 0, None, NONE, mem, C.byref(out), C.byref(count))
        refused(b"null sites", pa, 6, 0, 4, None, 9, mem, C.byref(out), C.byref(count))
        for n in (2 ** 32 - 1, 2 ** 32, 2 ** 63):
            refused(b"%d sites are too many" % n, pa, 6, 0, n, capi.ptr(sites), NONE, mem, C.byref(out), C.byref(count))
    for mem in (-1, 2, 7):
        refused(b"bad mem kind", pa, 6, 0, 4, capi.ptr(sites), NONE, mem, C.byref(out), C.byref(count))
    assert out.value == 0x1234 and count.value == 99 and not any(a)
    # the pieces' cells: NULL labels, labels that are not a fracture's (zero bytes say so), a bad mem kind
    for i in range(128):
        c[i] = 0x01010101
    got = np.full(4, 7, np.uint32)
    for mem in (H, D):
        assert L.vrc_fracture_piece_sites(None, 0, 4, capi.ptr(got), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_fracture_piece_sites: null labels")
        assert L.vrc_fracture_piece_sites(pa, 0, 4, capi.ptr(got), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_fracture_piece_sites: not fracture labels"), L.vrc_last_error()
        assert L.vrc_fracture_piece_sites(pc, 0, 4, None, mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_fracture_piece_sites: null buffer"), L.vrc_last_error()
    assert L.vrc_fracture_piece_sites(pc, 0, 4, capi.ptr(got), 5, None) == -1
    assert b"bad mem kind" in L.vrc_last_error()
    assert (got == 7).all() and all(v == 0x01010101 for v in c)


def test_python_arguments(built):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume.__new__(vrc.VoxelVolume)
    volume._h, volume.depth, volume.device = None, 4, 0
    with pytest.raises(ValueError, match="negative radius"):
        volume.fracture([[1, 2, 3]], max_distance=-1)
    with pytest.raises(vrc.VrcError, match="vrc_fracture_label"):
        volume.fracture(np.zeros((0, 3), np.int32))


def test_host_adapter_with_fracture_compiles(built):
    """HipVoxelVolume::fracture and HipVoxelLabels::pieceSites in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world) {\n'
           '    const std::vector<int32_t> sites = {1, 2, 3, 4, 5, 6};\n'
           '    vrc_host::HipVoxelLabels shards = world.fracture(sites, 6, false, 12);\n'
           '    vrc_host::HipVoxelLabels all = world.fracture(sites);\n'
           '    const std::vector<uint32_t> cells = shards.pieceSites();\n'
           '    return cells.size() + all.pieceSites(1, 2).size() + shards.count();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
