"""vrc_volume_xor_mesh on a machine without a GPU: the yardstick of the GPU tests itself -- the numpy model of
tests/voxelize_model.py against facts that need no model (boxes, a fan of triangles, an exact orientation test of random
tetrahedra) --, the refusals that need no device, the quantisation of VoxelVolume.voxelizeMesh, the mesh helpers and the
C++ host adapter under a plain C++14 compiler."""
import ctypes as C
import os

import numpy as np
import pytest

import voxelize_model as M
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def box_tris(lo, hi):
    """12 triangles (fixed point) of the box with corners lo, hi given in voxels (halves allowed)"""
    from cpuvoxelraycaster_amd import scenes
    verts, faces = scenes.box_mesh(lo, hi)
    return M.soup(M.quantise(verts), faces)


def test_integer_box_is_its_slice():
    """A box with integer corners gives exactly the voxels fill_boxes would set -- in any triangle order, with any mix of
    windings, and also where it sticks out of the volume."""
    S = 16
    rng = np.random.default_rng(1)
    for lo, hi in (((2, 3, 4), (9, 5, 15)), ((0, 0, 0), (16, 16, 16)), ((-3, 5, -2), (4, 20, 7)), ((5, 5, 5), (6, 6, 6))):
        want = np.zeros((S, S, S), np.uint8)
        want[max(lo[0], 0):hi[0], max(lo[1], 0):hi[1], max(lo[2], 0):hi[2]] = 1
        tris = box_tris(lo, hi)
        assert np.array_equal(M.xor_mesh(S, tris), want), (lo, hi)
        for _ in range(4):
            t = tris[rng.permutation(12)].reshape(-1, 3, 3)
            flip = rng.random(12) < 0.5
            t[flip] = t[flip][:, ::-1, :]                              # reversed winding
            t = np.roll(t, int(rng.integers(0, 3)), axis=1)            # another first vertex
            assert np.array_equal(M.xor_mesh(S, t.reshape(-1, 9)), want), (lo, hi)


def test_half_voxel_box_is_a_translated_box():
    """Faces, edges and corners through voxel centres: 8 x 5 x 28 voxels, one solid box, no doubled or missing layer."""
    S = 32
    got = M.xor_mesh(S, box_tris((2.5, 3.5, 1.5), (10.5, 8.5, 29.5)))
    assert int(got.sum()) == 8 * 5 * 28
    xyz = np.argwhere(got)
    assert tuple(xyz.max(axis=0) - xyz.min(axis=0) + 1) == (8, 5, 28)
    assert np.all(xyz.min(axis=0) >= (2, 3, 1)) and np.all(xyz.max(axis=0) <= (10, 8, 29))


def fan(height_units, mirror_x=False, mirror_y=False, swap=False):
    """A flat 9 x 9 square at z = height_units / 64 made of four triangles that meet at the centre of column (4, 4); its
    diagonals run through column centres.  Mirrored / transposed copies turn every edge into every orientation."""
    u = M.UNIT
    corners = [(0, 0), (9 * u, 0), (9 * u, 9 * u), (0, 9 * u)]
    centre = (4 * u + M.HALF, 4 * u + M.HALF)
    tris = []
    for i in range(4):
        tri = [centre, corners[i], corners[(i + 1) % 4]]
        out = []
        for x, y in tri:
            x, y = (9 * u - x if mirror_x else x), (9 * u - y if mirror_y else y)
            x, y = (y, x) if swap else (x, y)
            out += [x, y, height_units]
        tris.append(out)
    return np.array(tris, np.int32)


FAN_VARIANTS = [(mx, my, sw) for mx in (False, True) for my in (False, True) for sw in (False, True)]


def test_fan_covers_every_column_once():
    """Shared edges through column centres belong to exactly one of the two triangles, and the shared apex on a column
    centre to exactly one of the four.  Heights: between centres, and planes exactly through voxel centres."""
    S = 16
    for mx, my, sw in FAN_VARIANTS:
        for h, k in ((5 * 64, 5), (5 * 64 + 32, 5), (5 * 64 + 33, 6), (32, 0), (33, 1), (40 * 64, 16), (-64, 0)):
            got = M.xor_mesh(S, fan(h, mx, my, sw))
            want = np.zeros((S, S, S), np.uint8)
            want[0:9, 0:9, 0:k] = 1
            assert np.array_equal(got, want), (mx, my, sw, h)


def orient(a, b, c, p):
    """sign of det[b - a, c - a, p - a], p an (..., 3) int64 array; products stay below 2^60 for |coordinates| < 2^12"""
    u, w = b - a, c - a
    n = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]], np.int64)
    return np.sign((p - a) @ n)


def test_random_tetrahedra_against_an_exact_orientation_test():
    """30 random tetrahedra around a 16^3 volume, partly outside it: every voxel centre strictly inside one is set, every
    centre strictly outside is not (centres exactly on a face are left to the tie rule)."""
    S = 16
    rng = np.random.default_rng(2)
    centres = (np.stack(np.meshgrid(*[np.arange(S)] * 3, indexing="ij"), axis=-1).astype(np.int64) * M.UNIT + M.HALF)
    interior = 0
    for _ in range(30):
        v = rng.integers(-3 * M.UNIT, (S + 3) * M.UNIT, (4, 3)).astype(np.int64)
        if orient(v[0], v[1], v[2], v[3][None, :])[0] == 0:
            continue
        faces = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]
        got = M.xor_mesh(S, M.soup(v, faces))
        signs = []
        for f in faces:
            other = v[({0, 1, 2, 3} - set(f)).pop()]
            signs.append(orient(v[f[0]], v[f[1]], v[f[2]], centres) * orient(v[f[0]], v[f[1]], v[f[2]], other[None, :])[0])
        signs = np.stack(signs)
        inside, outside = np.all(signs > 0, axis=0), np.any(signs < 0, axis=0)
        assert np.all(got[inside] == 1) and np.all(got[outside] == 0)
        interior += int(inside.sum())
    assert interior > 2000


def test_model_drops_out_of_range_and_vertical_triangles():
    S = 8
    sheet = np.array([[0, 0, 200, 512, 0, 200, 0, 512, 200]], np.int32)
    base = M.xor_mesh(S, sheet)
    assert base.sum() > 0
    far = np.array([[0, 0, 200, (1 << 17) + 1, 0, 200, 0, 512, 200], [0, 0, 200, 512, 0, 200, 0, -(1 << 17) - 1, 200]], np.int32)
    vertical = np.array([[0, 0, 0, 512, 0, 0, 512, 0, 512], [64, 64, 64, 64, 64, 64, 64, 64, 64], [0, 0, 0, 64, 64, 64, 128, 128, 128]], np.int32)
    assert np.array_equal(M.xor_mesh(S, np.concatenate([far, sheet, vertical])), base)
    edge = np.array([[0, 0, 200, 1 << 17, 0, 200, 0, 512, 200]], np.int32)              # exactly at the limit: applies
    assert M.xor_mesh(S, edge).sum() > 0


def test_xor_mesh_refusals_need_no_gpu(built):
    """NULL volume, NULL triangles with n > 0 and a bad memory kind are VRC_ERR_INVALID with the function's name before any
    HIP call and before the volume is read (the handle here is no volume at all); n == 0 is accepted the same way."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    assert capi.VRC_MESH_FRAC_BITS == 6 == M.FRAC
    fake = (C.c_uint64 * 64)()
    pv = C.cast(fake, C.c_void_p)
    tris = np.zeros(9, np.int32)
    cases = [(None, 1, capi.ptr(tris), 0), (None, 0, None, 0), (pv, 1, None, 0), (pv, 1, None, 1),
             (pv, 1, capi.ptr(tris), 2), (pv, 1, capi.ptr(tris), -1), (pv, 0, None, 7)]
    for v, n, t, mem in cases:
        assert L.vrc_volume_xor_mesh(v, n, t, mem, None) == -1, (n, mem)
        assert L.vrc_last_error().startswith(b"vrc_volume_xor_mesh"), L.vrc_last_error()
    assert L.vrc_volume_xor_mesh(pv, 0, None, 0, None) == 0
    assert L.vrc_volume_xor_mesh(pv, 0, capi.ptr(tris), 1, None) == 0
    assert not any(fake)
    # the scratch query refuses NULL the same way
    n = C.c_uint64(7)
    assert L.vrc_volume_edit_scratch_bytes(None, C.byref(n)) == -1 and L.vrc_volume_edit_scratch_bytes(pv, None) == -1
    assert L.vrc_last_error().startswith(b"vrc_volume_edit_scratch_bytes") and n.value == 7


def test_quantisation_keeps_shared_vertices_shared():
    """voxelizeMesh quantises every VERTEX once: in the soup, all copies of a vertex are one integer point and every edge
    appears exactly twice, once in each direction -- the mesh stays closed whatever the scale and offset."""
    from cpuvoxelraycaster_amd import scenes
    from cpuvoxelraycaster_amd.raycaster import VoxelVolume
    for sub, n_faces in ((0, 20), (1, 80), (2, 320), (3, 1280)):
        verts, faces = scenes.icosphere(sub)
        assert faces.shape == (n_faces, 3) and len(verts) == 10 * 4 ** sub + 2
        assert np.allclose(np.linalg.norm(verts, axis=1), 1.0)
        fixed = VoxelVolume.quantiseMesh(verts, 13.37, (20.123, 17.5, 9.99))
        assert fixed.dtype == np.int32 and np.array_equal(fixed, M.quantise(verts, 13.37, (20.123, 17.5, 9.99)))
        soup = M.soup(fixed, faces).reshape(-1, 3, 3)
        edges = {}
        for tri in soup:
            for i in range(3):
                key = (tuple(tri[i]), tuple(tri[(i + 1) % 3]))
                edges[key] = edges.get(key, 0) + 1
        assert all(c == 1 for c in edges.values())
        assert all((q, p) in edges for p, q in edges)
        # outward winding: every face's normal points away from the centre
        t = verts[faces]
        assert np.all(np.einsum("ij,ij->i", np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), t.sum(axis=1)) > 0)
    with pytest.raises(Exception, match="2048"):
        VoxelVolume.quantiseMesh([[0.0, 0.0, 2049.0]])
    verts, faces = scenes.box_mesh((1, 2, 3), (4, 6, 8))
    t = verts[faces]
    assert np.all(np.einsum("ij,ij->i", np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), t.mean(axis=1) - (2.5, 4.0, 5.5)) > 0)


def test_icosphere_solid_is_a_ball():
    """The model on a closed curved mesh: every centre well inside the inscribed sphere is set, none outside the unit one."""
    from cpuvoxelraycaster_amd import scenes
    S, r, c = 32, 12.3, (15.2, 16.9, 14.4)
    verts, faces = scenes.icosphere(2)
    got = M.xor_mesh(S, M.soup(M.quantise(verts, r, c), faces))
    g = np.stack(np.meshgrid(*[np.arange(S) + 0.5] * 3, indexing="ij"), axis=-1)
    d = np.linalg.norm(g - np.asarray(c), axis=-1)
    assert np.all(got[d < 0.95 * r - 0.1] == 1) and np.all(got[d > r + 0.1] == 0)


def test_host_adapter_with_mesh_compiles(built):
    """HipVoxelVolume::xorMesh / voxelizeMesh / stampMesh in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, const std::vector<double>& verts, const std::vector<uint32_t>& faces) {\n'
           '    world.xorMesh(std::vector<int32_t>(9, 0));\n'
           '    world.xorMeshDevice(0, nullptr);\n'
           '    world.voxelizeMesh(verts, faces);\n'
           '    world.voxelizeMesh(verts, faces, 2.0, 1.0, 2.0, 3.0);\n'
           '    world.stampMesh(verts, faces);\n'
           '    world.stampMesh(verts, faces, VRC_COPY_ANDNOT, 2.0, 1.0, 2.0, 3.0);\n'
           '    return world.solidCount() + vrc_host::HipVoxelVolume::quantiseMesh(verts).size();\n'
           '}\nint main(){ return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
    main = os.path.join(ROOT, "tests", "cpp", "voxel_mesh_main.cpp")
    check_cpp_syntax(main, strict=True)
