"""Connected components on a machine without a GPU: the refusals that need no device, the record's size, the C++ host
adapter with HipVoxelLabels under a plain C++14 compiler, and the yardstick of the GPU tests itself -- the numpy model of
tests/components_model.py against a plain breadth-first search that visits the voxels in key order."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest

import components_model as model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key_of(S, x, y, z):
    n = S // 2
    return 8 * (((x >> 1) * n + (y >> 1)) * n + (z >> 1)) + (z & 1) * 4 + (y & 1) * 2 + (x & 1)


def bfs_label(medium, connectivity, through_empty):
    """The definition, voxel by voxel: the voxels of M in ascending key order; one not yet visited is the representative of
    the next component, which a breadth-first search collects.  Returns (ids, list of (first, lo, hi, voxels))."""
    S = medium.shape[0]
    M = (medium == 0) if through_empty else (medium != 0)
    steps = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    assert len(steps) == connectivity
    ids = np.full((S, S, S), model.NO_COMPONENT, np.uint32)
    records = []
    voxels = sorted((key_of(S, x, y, z), x, y, z) for x, y, z in np.argwhere(M).tolist())
    for _, x, y, z in voxels:
        if ids[x, y, z] != model.NO_COMPONENT:
            continue
        cid = len(records)
        ids[x, y, z] = cid
        queue, members = deque([(x, y, z)]), []
        while queue:
            p = queue.popleft()
            members.append(p)
            for d in steps:
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if min(q) < 0 or max(q) >= S or not M[q] or ids[q] != model.NO_COMPONENT:
                    continue
                ids[q] = cid
                queue.append(q)
        m = np.array(members)
        records.append(((x, y, z), tuple(m.min(axis=0)), tuple(m.max(axis=0) + 1), len(members)))
    return ids, records


@pytest.mark.parametrize("through_empty", [False, True])
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("S", [4, 8, 16])
def test_model_against_breadth_first_search(S, connectivity, through_empty):
    rng = np.random.default_rng(900 + S + connectivity + int(through_empty))
    densities = (0.2, 0.31, 0.4, 0.7) if connectivity == 6 else (0.05, 0.1, 0.15, 0.5)
    pieces = 0
    for density in densities:
        in_m = rng.random((S, S, S)) < density
        medium = (~in_m if through_empty else in_m).astype(np.uint8)
        ids, rec = model.label(medium, connectivity, through_empty)
        want_ids, want_rec = bfs_label(medium, connectivity, through_empty)
        assert np.array_equal(ids, want_ids), (S, connectivity, through_empty, density)
        assert len(rec) == len(want_rec)
        for r, (first, lo, hi, count) in zip(rec, want_rec):
            assert tuple(r["first"]) == first and tuple(r["lo"]) == lo and tuple(r["hi"]) == hi
            assert int(r["voxels"]) == count and int(r["reserved"]) == 0
        # the id order is the order of the representatives' keys
        firsts = [key_of(S, *map(int, r["first"])) for r in rec]
        assert firsts == sorted(firsts)
        pieces += len(rec)
    assert pieces > len(densities)


def test_model_on_empty_and_full():
    for S in (4, 8):
        ids, rec = model.label(np.zeros((S, S, S), np.uint8))
        assert len(rec) == 0 and (ids == model.NO_COMPONENT).all()
        ids, rec = model.label(np.zeros((S, S, S), np.uint8), 26, True)
        assert len(rec) == 1 and not ids.any()
        assert tuple(rec[0]["first"]) == (0, 0, 0) and tuple(rec[0]["lo"]) == (0, 0, 0) and tuple(rec[0]["hi"]) == (S, S, S)
        assert int(rec[0]["voxels"]) == S ** 3


def test_model_select_and_despeckle():
    vol = np.zeros((8, 8, 8), np.uint8)
    vol[0:3, 0:3, 0:3] = 1
    vol[5, 5, 5] = 1
    vol[7, 7, 6:8] = 1
    ids, rec = model.label(vol)
    assert [int(v) for v in rec["voxels"]] == [27, 1, 2]
    assert np.array_equal(model.select(ids, [1, 1, 1]), vol)
    assert int(model.select(ids, [0, 1, 0]).sum()) == 1 and model.select(ids, [0, 1, 0])[5, 5, 5] == 1
    kept = model.despeckle(vol, 2)
    assert int(kept.sum()) == 29 and kept[5, 5, 5] == 0


def test_component_record_layout(built):
    from cpuvoxelraycaster_amd import capi
    assert capi.COMPONENT_DTYPE.itemsize == 48
    assert capi.COMPONENT_DTYPE == model.RECORD
    assert [capi.COMPONENT_DTYPE.fields[k][1] for k in ("first", "lo", "hi", "reserved", "voxels")] == [0, 12, 24, 36, 40]
    assert capi.VRC_NO_COMPONENT == model.NO_COMPONENT == 0xFFFFFFFF


def test_component_refusals_need_no_gpu(built):
    """NULL handles, a connectivity other than 6 / 26, a `through` other than 0 / 1, an unknown op, a bad mem kind and
    labels against a volume of another depth are VRC_ERR_INVALID with the function's name before any HIP call: the
    handles here are not volumes or labels at all, and nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b = (C.c_uint32 * 128)(), (C.c_uint32 * 128)()        # 512 zero bytes each: "depth 0 on device 0" whatever the layout
    pa, pb = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    out, count = C.c_void_p(0x55), C.c_uint64(7)
    for medium, conn, through, o in [(None, 6, 0, C.byref(out)), (pa, 6, 0, None), (pa, 0, 0, C.byref(out)), (pa, 18, 0, C.byref(out)),
                                     (pa, 7, 1, C.byref(out)), (pa, 6, 2, C.byref(out)), (pa, 26, -1, C.byref(out))]:
        for cnt in (None, C.byref(count)):
            assert L.vrc_volume_label_components(medium, conn, through, o, cnt) == -1, (conn, through)
            assert L.vrc_last_error().startswith(b"vrc_volume_label_components"), L.vrc_last_error()
    assert out.value == 0x55 and count.value == 7

    assert L.vrc_labels_destroy(None) == 0
    assert L.vrc_labels_count(None) == 0 and L.vrc_labels_depth(None) == 0 and L.vrc_labels_bytes(None) == 0
    rec = np.zeros(2, capi.COMPONENT_DTYPE)
    xyz, ids = np.zeros(3, np.uint32), np.full(1, 9, np.uint32)
    keep = np.ones(4, np.uint8)
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_labels_components(None, 0, 2, capi.ptr(rec), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_labels_components")
        assert L.vrc_labels_at(None, 1, capi.ptr(xyz), capi.ptr(ids), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_labels_at")
        assert L.vrc_labels_select(None, capi.ptr(keep), pb, capi.VRC_COPY_REPLACE, mem, None) == -1
        assert L.vrc_labels_select(pa, capi.ptr(keep), None, capi.VRC_COPY_REPLACE, mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_labels_select")
        for op in (-1, 3, 26):
            assert L.vrc_labels_select(pa, capi.ptr(keep), pb, op, mem, None) == -1
            assert L.vrc_last_error().startswith(b"vrc_labels_select: bad op"), L.vrc_last_error()
    for mem in (-1, 2, 7):
        assert L.vrc_labels_components(pa, 0, 2, capi.ptr(rec), mem, None) == -1
        assert L.vrc_labels_at(pa, 1, capi.ptr(xyz), capi.ptr(ids), mem, None) == -1
        assert L.vrc_labels_select(pa, capi.ptr(keep), pb, capi.VRC_COPY_OR, mem, None) == -1
        assert b"bad mem kind" in L.vrc_last_error()
    assert L.vrc_labels_components(pa, 0, 2, None, capi.VRC_MEM_HOST, None) == -1     # capacity without a buffer
    # a volume whose every field differs from the labels': a depth (or device) mismatch
    for i in range(128):
        b[i] = 0x01010101
    for op in (capi.VRC_COPY_REPLACE, capi.VRC_COPY_OR, capi.VRC_COPY_ANDNOT):
        assert L.vrc_labels_select(pa, capi.ptr(keep), pb, op, capi.VRC_MEM_HOST, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_labels_select: labels"), L.vrc_last_error()
    assert not any(a) and all(v == 0x01010101 for v in b)
    assert not rec.view(np.uint8).any() and ids[0] == 9


def test_host_adapter_with_labels_compiles(built):
    """HipVoxelLabels and HipVoxelVolume::labelComponents / removeSmallPieces in the header-only adapter: C++14, no GLM,
    no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world) {\n'
           '    vrc_host::HipVoxelLabels labels = world.labelComponents(26, false);\n'
           '    std::vector<vrc_component> records = labels.components();\n'
           '    std::vector<uint8_t> keep(labels.count(), 1);\n'
           '    vrc_host::HipVoxelVolume piece(world.depth());\n'
           '    labels.select(keep, piece, VRC_COPY_REPLACE);\n'
           '    const uint32_t xyz[3] = {1, 2, 3};\n'
           '    std::vector<uint32_t> ids = labels.at(xyz, 1);\n'
           '    return world.removeSmallPieces(8) + records.size() + ids[0] + labels.bytes();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
