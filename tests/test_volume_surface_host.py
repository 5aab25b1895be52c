"""vrc_volume_extract_surface on a machine without a GPU: the yardstick of the GPU tests itself -- the numpy model of
tests/surface_model.py against a per-voxel loop and, through the voxeliser's model, against the round trip (the exposed
faces of a voxel set are a closed mesh whose solid voxelisation is the voxel set) --, the quad mesh and OBJ helpers, the
refusals that need no device and the C++ host adapter under a plain C++14 compiler."""
import ctypes as C
import os

import numpy as np
import pytest

import surface_model as F
import voxelize_model as M
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_field(S, density, seed):
    return (np.random.default_rng(seed).random((S, S, S)) < density).astype(np.uint8)


def corner_fields(S):
    for x in (0, S - 1):
        for y in (0, S - 1):
            for z in (0, S - 1):
                V = np.zeros((S, S, S), np.uint8)
                V[x, y, z] = 1
                yield V


def checkerboard(S):
    g = np.indices((S, S, S)).sum(axis=0)
    return (g & 1).astype(np.uint8)


def faces_by_loop(V, closed):
    """the rule voxel by voxel, and the order by sorting Python tuples"""
    S = V.shape[0]
    n = S // 2
    found = []
    for x in range(S):
        for y in range(S):
            for z in range(S):
                if not V[x, y, z]:
                    continue
                key = 8 * (((x >> 1) * n + (y >> 1)) * n + (z >> 1)) + (z & 1) * 4 + (y & 1) * 2 + (x & 1)
                for d in range(6):
                    q = [x, y, z]
                    q[d >> 1] += 1 if d & 1 else -1
                    inside = 0 <= q[d >> 1] < S
                    neighbour = V[q[0], q[1], q[2]] if inside else (0 if closed else 1)
                    if not neighbour:
                        found.append((key >> 5, d, key & 31, x, y, z))
    found.sort()
    return np.array([(x, y, z, d) for _, d, _, x, y, z in found], np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("S", [4, 8])
@pytest.mark.parametrize("closed", [True, False])
def test_model_equals_the_per_voxel_loop(S, closed):
    for density in (0.2, 0.5, 0.9):
        V = random_field(S, density, 10 * S + int(density * 10))
        got = F.faces(V, closed)
        assert got.dtype == np.uint32 and np.array_equal(got, faces_by_loop(V, closed)), (S, closed, density)
        assert np.array_equal(F.direction_counts(got), np.bincount(got[:, 3], minlength=6))
        assert F.word_direction_counts(got, S).sum() == got.shape[0]


def test_round_trip_through_the_voxeliser_model():
    """xor_mesh(triangles(faces(V))) == V: face corners lie at multiples of 64 units and voxel centres at + 32, so no tie
    rule of the voxeliser is exercised"""
    fields = [random_field(S, density, 100 * S + int(density * 10)) for S in (4, 8, 16) for density in (0.1, 0.5, 1.0)]
    fields += list(corner_fields(4)) + list(corner_fields(8)) + [checkerboard(4), checkerboard(8)]
    for V in fields:
        S = V.shape[0]
        tris = F.triangles(F.faces(V, True))
        assert tris.dtype == np.int32 and tris.shape[1] == 9 and tris.min() >= 0 and tris.max() <= 64 * S
        assert np.array_equal(M.xor_mesh(S, tris), V), (S, int(V.sum()))
    assert F.faces(checkerboard(8)).shape[0] == 6 * checkerboard(8).sum()


def test_triangle_normals_point_out_of_the_voxel():
    V = random_field(8, 0.4, 5)
    faces = F.faces(V, True)
    t = F.triangles(faces).reshape(-1, 2, 3, 3).astype(np.int64)
    normal = np.cross(t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 0])      # (faces, 2, 3)
    axis, side = faces[:, 3] >> 1, faces[:, 3] & 1
    for k in range(2):
        assert np.array_equal(np.count_nonzero(normal[:, k], axis=1), np.ones(len(faces)))
        along = normal[np.arange(len(faces)), k, axis]
        assert np.array_equal(np.sign(along), np.where(side == 1, 1, -1))
    # and the two triangles of a face tile its unit square: areas 64^2 / 2 each, all corners on the face's plane
    assert np.all(np.abs(normal).sum(axis=2) == 64 * 64)
    plane = 64 * (faces[np.arange(len(faces)), axis].astype(np.int64) + side)
    assert np.all(t[np.arange(len(faces)), :, :, axis].reshape(len(faces), -1) == plane[:, None])


@pytest.mark.parametrize("S", [4, 8, 16])
def test_full_and_empty_volumes(S):
    full = np.ones((S, S, S), np.uint8)
    assert F.faces(full, False).shape == (0, 4)
    closed = F.faces(full, True)
    assert closed.shape[0] == 6 * S * S and np.array_equal(F.direction_counts(closed), np.full(6, S * S))
    assert F.faces(np.zeros((S, S, S), np.uint8), True).shape == (0, 4)
    assert F.triangles(np.zeros((0, 4), np.uint32)).shape == (0, 9)


def quad_edges(quads):
    edges = {}
    for q in quads.tolist():
        for k in range(4):
            e = (min(q[k], q[(k + 1) % 4]), max(q[k], q[(k + 1) % 4]))
            edges[e] = edges.get(e, 0) + 1
    return edges


def test_quad_mesh_from_faces():
    from cpuvoxelraycaster_amd.raycaster import VoxelVolume
    for V in (random_field(8, 0.3, 77), checkerboard(4), np.ones((4, 4, 4), np.uint8)):
        faces = F.faces(V, True)
        verts, quads = VoxelVolume.meshFromFaces(faces)
        assert verts.dtype == np.int32 and quads.dtype == np.int64 and quads.shape == (faces.shape[0], 4)
        assert len(np.unique(verts, axis=0)) == len(verts)                      # corners are deduplicated
        assert set(np.unique(quads)) == set(range(len(verts)))                  # and every one of them is used
        # each quad's corners are its face's corners -- the four distinct corners of its two triangles -- wound outwards
        t = F.triangles(faces).reshape(-1, 6, 3)
        c = 64 * verts[quads].astype(np.int64)
        for i in range(len(faces)):
            assert {tuple(p) for p in c[i].tolist()} == {tuple(p) for p in t[i].tolist()} and len({tuple(p) for p in c[i].tolist()}) == 4
        axis, side = faces[:, 3] >> 1, faces[:, 3] & 1
        for k in range(4):
            turn = np.cross(c[:, (k + 1) % 4] - c[:, k], c[:, (k + 2) % 4] - c[:, (k + 1) % 4])
            assert np.array_equal(np.sign(turn[np.arange(len(faces)), axis]), np.where(side == 1, 1, -1))
        # closed: every edge is used by an even number of quads
        assert all(c % 2 == 0 for c in quad_edges(quads).values())
    verts, quads = VoxelVolume.meshFromFaces(np.zeros((0, 4), np.uint32))
    assert verts.shape == (0, 3) and quads.shape == (0, 4)
    # the open form of a slab on a wall is not closed
    V = np.zeros((4, 4, 4), np.uint8)
    V[0] = 1
    _, quads = VoxelVolume.meshFromFaces(F.faces(V, False))
    assert any(c % 2 for c in quad_edges(quads).values())


def test_write_obj_reads_back(tmp_path):
    from cpuvoxelraycaster_amd import scenes
    from cpuvoxelraycaster_amd.raycaster import VoxelVolume
    verts, quads = VoxelVolume.meshFromFaces(F.faces(random_field(8, 0.3, 3), True))
    path = tmp_path / "surface.obj"
    scenes.write_obj(str(path), verts, quads)
    v, f = [], []
    for line in path.read_text().splitlines():
        kind, *rest = line.split()
        assert kind in ("v", "f")
        (v if kind == "v" else f).append([int(q) for q in rest])
    assert np.array_equal(np.array(v, np.int32), verts)
    assert np.array_equal(np.array(f, np.int64) - 1, quads)


def test_surface_refusals_need_no_gpu(built):
    """NULL volume, unknown format or memory kind, NULL out with a capacity and NULL counts are VRC_ERR_INVALID with the
    function's name before any HIP call and before the volume is read (the handle here is no volume at all)."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    assert (capi.VRC_FACE_XN, capi.VRC_FACE_XP, capi.VRC_FACE_YN, capi.VRC_FACE_YP, capi.VRC_FACE_ZN, capi.VRC_FACE_ZP) == tuple(range(6))
    assert (capi.VRC_SURFACE_FACES, capi.VRC_SURFACE_TRIANGLES) == (0, 1)
    fake = (C.c_uint64 * 64)()
    pv = C.cast(fake, C.c_void_p)
    out = np.zeros(64, np.uint32)
    total = C.c_uint64(7)
    cases = [(None, 0, 0, capi.ptr(out), 0), (pv, 2, 1, capi.ptr(out), 0), (pv, -1, 1, capi.ptr(out), 1), (pv, 0, 1, capi.ptr(out), 2),
             (pv, 1, 1, capi.ptr(out), -1), (pv, 0, 1, None, 0), (pv, 1, 5, None, 1)]
    for v, fmt, cap, o, mem in cases:
        assert L.vrc_volume_extract_surface(v, 1, fmt, 0, cap, o, C.byref(total), mem, None) == -1, (fmt, cap, mem)
        assert L.vrc_last_error().startswith(b"vrc_volume_extract_surface"), L.vrc_last_error()
    counts = np.zeros(6, np.uint64)
    assert L.vrc_volume_surface_count(None, 1, capi.ptr(counts)) == -1 and L.vrc_last_error().startswith(b"vrc_volume_surface_count")
    assert L.vrc_volume_surface_count(pv, 1, None) == -1 and L.vrc_last_error().startswith(b"vrc_volume_surface_count")
    assert total.value == 7 and not any(fake) and not out.any() and not counts.any()


def test_host_adapter_with_surface_compiles(built):
    """HipVoxelVolume::surfaceCount / surfaceFaces / surfaceTriangles / extractSurfaceDevice / toObj in the header-only
    adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, void* dev, uint64_t* total_dev) {\n'
           '    const std::vector<uint64_t> counts = world.surfaceCount();\n'
           '    const std::vector<uint32_t> faces = world.surfaceFaces(false, 3, 10);\n'
           '    const std::vector<int32_t> tris = world.surfaceTriangles();\n'
           '    world.extractSurfaceDevice(VRC_SURFACE_TRIANGLES, 0, 100, dev, total_dev);\n'
           '    world.extractSurfaceDevice(VRC_SURFACE_FACES, 0, 100, dev, nullptr, false, nullptr);\n'
           '    return counts[VRC_FACE_ZP] + faces.size() + tris.size() + world.toObj("world.obj") + world.toObj("open.obj", false);\n'
           '}\nint main(){ return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
    main = os.path.join(ROOT, "tests", "cpp", "voxel_surface_main.cpp")
    check_cpp_syntax(main, strict=True)
