"""vrc_extract_rects on a machine without a GPU: the yardstick of the GPU tests itself -- the numpy model of
tests/rect_model.py against a per-cell restatement of the definition (for every exposed face, find its rectangle by
scanning outwards), the exact single cover of every face mask, and, through the voxeliser's model, the round trip --, the
packing, the merged quad mesh, the refusals that need no device and the C++ host adapter under a plain C++14 compiler."""
import ctypes as C
import os

import numpy as np
import pytest

import rect_model as R
import surface_model as F
import voxelize_model as M
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_field(S, density, seed):
    return (np.random.default_rng(seed).random((S, S, S)) < density).astype(np.uint8)


def checkerboard(S):
    return (np.indices((S, S, S)).sum(axis=0) & 1).astype(np.uint8)


def ball(S, radius):
    g = np.indices((S, S, S)).astype(np.int64) - S // 2
    return ((g ** 2).sum(axis=0) <= radius * radius).astype(np.uint8)


def height_field(S, seed):
    rng = np.random.default_rng(seed)
    h = (S // 2 + 6 * np.sin(np.arange(S) / 7.0)[:, None] + 5 * np.cos(np.arange(S) / 5.0)[None, :] + rng.integers(0, 2, (S, S))).astype(np.int64)
    return (np.arange(S)[None, :, None] < h[:, None, :]).astype(np.uint8)       # solid below y = h(x, z)


def rects_by_loop(V, closed):
    """the definition cell by cell: the rectangle of every exposed face, found by scanning outwards from it; the set of
    them, ordered by sorting Python tuples"""
    S = V.shape[0]
    mask = R.face_masks(V, closed)
    found = set()
    for d in range(6):
        a = d >> 1
        s, r = R.STACK[a], R.RUN[a]
        m = mask[d].transpose(a, s, r)

        def run_of(ca, cs, cr):
            """the maximal run of row (ca, cs) that holds cr, or None"""
            if not (0 <= cs < S) or not m[ca, cs, cr]:
                return None
            r0, r1 = cr, cr + 1
            while r0 > 0 and m[ca, cs, r0 - 1]:
                r0 -= 1
            while r1 < S and m[ca, cs, r1]:
                r1 += 1
            return r0, r1

        for ca, cs, cr in np.argwhere(m).tolist():
            run = run_of(ca, cs, cr)
            s0 = cs
            while run_of(ca, s0 - 1, cr) == run:
                s0 -= 1
            s1 = cs + 1
            while run_of(ca, s1, cr) == run:
                s1 += 1
            found.add((d, ca, s0, run[0], run[1] - run[0], s1 - s0))
    out = []
    for d, ca, s0, r0, nr, ns in sorted(found):
        a = d >> 1
        c = [0, 0, 0]
        c[a], c[R.STACK[a]], c[R.RUN[a]] = ca, s0, r0
        out.append(c + [d | (nr - 1) << 8 | (ns - 1) << 20])
    return np.array(out, np.uint32).reshape(-1, 4)


def check_cover(V, closed, records):
    S = V.shape[0]
    assert np.array_equal(R.cover(records, S), R.face_masks(V, closed).astype(np.int64))


@pytest.mark.parametrize("S", [4, 8])
@pytest.mark.parametrize("closed", [True, False])
def test_model_equals_the_per_cell_definition(S, closed):
    for density in (0.2, 0.5, 0.9):
        V = random_field(S, density, 10 * S + int(density * 10))
        got = R.rects(V, closed)
        assert got.dtype == np.uint32 and np.array_equal(got, rects_by_loop(V, closed)), (S, closed, density)
        assert np.array_equal(R.ordered(got[::-1]), got)
        assert R.direction_counts(got).sum() == got.shape[0]
    for V in (ball(8, 3), checkerboard(S), np.ones((S, S, S), np.uint8)):
        assert np.array_equal(R.rects(V, closed), rects_by_loop(V, closed))


def test_every_face_is_covered_exactly_once():
    fields = [random_field(S, density, 7 * S + int(density * 10)) for S in (4, 8, 16, 32) for density in (0.1, 0.5, 0.9)]
    box = np.zeros((32, 32, 32), np.uint8)
    box[3:20, 5:9, 11:30] = 1
    fields += [ball(32, 13), box, np.ones((32, 32, 32), np.uint8), checkerboard(8), height_field(64, 3)]
    for V in fields:
        for closed in (True, False):
            records = R.rects(V, closed)
            check_cover(V, closed, records)
            assert records.shape[0] <= F.faces(V, closed).shape[0]


def test_counts_against_faces():
    board = checkerboard(8)
    assert R.rects(board).shape[0] == F.faces(board).shape[0] == 6 * board.sum()
    full = np.ones((32, 32, 32), np.uint8)
    assert R.rects(full, False).shape == (0, 4)
    u = R.unpack(R.rects(full, True))
    assert u.shape == (6, 6) and np.all(u[:, 4:] == 32) and np.array_equal(u[:, 3], np.arange(6))
    assert np.array_equal(u[:, :3], [[0, 0, 0], [31, 0, 0], [0, 0, 0], [0, 31, 0], [0, 0, 0], [0, 0, 31]])
    assert R.rects(np.zeros((8, 8, 8), np.uint8)).shape == (0, 4) and R.triangles(np.zeros((0, 4), np.uint32)).shape == (0, 9)
    b = ball(32, 13)
    assert R.rects(b).shape[0] < F.faces(b).shape[0]


def test_a_box_gives_six_records():
    rng = np.random.default_rng(11)
    for _ in range(12):
        lo = rng.integers(0, 12, 3)
        hi = lo + rng.integers(1, 5, 3)
        V = np.zeros((16, 16, 16), np.uint8)
        V[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
        u = R.unpack(R.rects(V, True))
        assert u.shape[0] == 6 and np.array_equal(u[:, 3], np.arange(6))
        size = hi - lo
        for x, y, z, d, nr, ns in u.tolist():
            a = d >> 1
            want = lo.copy()
            if d & 1:
                want[a] = hi[a] - 1
            assert [x, y, z] == want.tolist() and nr == size[R.RUN[a]] and ns == size[R.STACK[a]]


def test_identical_run_not_containing_run():
    """rows stacked along x on the +y faces of a one-voxel-thick sheet: [5, 20) above [5, 20) above [5, 21) gives heights 2
    and 1; a run that merely contains or overlaps the one before starts a rectangle of its own"""
    V = np.zeros((32, 32, 32), np.uint8)
    V[3, 7, 5:20] = V[4, 7, 5:20] = 1
    V[5, 7, 5:21] = 1
    V[6, 7, 6:21] = 1
    u = R.unpack(R.rects(V, False))
    top = u[u[:, 3] == 3]
    assert top.tolist() == [[3, 7, 5, 3, 15, 2], [5, 7, 5, 3, 16, 1], [6, 7, 6, 3, 15, 1]]


def test_round_trip_through_the_voxeliser_model():
    fields = [random_field(S, density, 100 * S + int(density * 10)) for S in (4, 8, 16) for density in (0.1, 0.5, 1.0)]
    fields += [ball(32, 13), checkerboard(8)]
    box = np.zeros((16, 16, 16), np.uint8)
    box[2:9, 0:16, 5:6] = 1
    fields.append(box)
    for V in fields:
        S = V.shape[0]
        tris = R.triangles(R.rects(V, True))
        assert tris.dtype == np.int32 and tris.shape[1] == 9 and tris.min() >= 0 and tris.max() <= 64 * S
        assert np.array_equal(M.xor_mesh(S, tris), V), (S, int(V.sum()))


def test_triangles_tile_the_rectangle_and_point_outwards():
    V = random_field(8, 0.6, 5)
    records = R.rects(V, True)
    u = R.unpack(records)
    t = R.triangles(records).reshape(-1, 2, 3, 3).astype(np.int64)
    normal = np.cross(t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 0])
    axis, side = u[:, 3] >> 1, u[:, 3] & 1
    rows = np.arange(len(u))
    for k in range(2):
        assert np.array_equal(np.count_nonzero(normal[:, k], axis=1), np.ones(len(u)))
        assert np.array_equal(np.sign(normal[rows, k, axis]), np.where(side == 1, 1, -1))
        assert np.array_equal(np.abs(normal[rows, k, axis]), 64 * 64 * u[:, 4] * u[:, 5])      # twice the triangle's area


def test_packing():
    rec = R.pack([[0, 1023, 0]], [3], [1024], [1024])
    assert rec.dtype == np.uint32 and rec[0, 3] == 3 | 1023 << 8 | 1023 << 20 and rec[0, 3] < 1 << 30
    assert R.unpack(rec).tolist() == [[0, 1023, 0, 3, 1024, 1024]]
    assert R.unpack(R.pack([[1, 2, 3]], [5], [1], [1024])).tolist() == [[1, 2, 3, 5, 1, 1024]]
    assert R.unpack(R.pack([[1, 2, 3]], [4], [1024], [1])).tolist() == [[1, 2, 3, 4, 1024, 1]]
    # a 1 x 1 rectangle's record is the face record, and its triangles are the face's
    board = checkerboard(8)
    records, faces = R.rects(board), F.faces(board)
    assert sorted(map(tuple, records.tolist())) == sorted(map(tuple, faces.tolist()))
    assert np.array_equal(R.triangles(records), F.triangles(records))
    from cpuvoxelraycaster_amd.raycaster import VoxelVolume
    assert np.array_equal(VoxelVolume.unpackRects(rec), R.unpack(rec))
    assert VoxelVolume.unpackRects(np.zeros((0, 4), np.uint32)).shape == (0, 6)


def test_merged_quad_mesh(tmp_path):
    from cpuvoxelraycaster_amd import scenes
    from cpuvoxelraycaster_amd.raycaster import VoxelVolume
    for V in (random_field(8, 0.6, 77), ball(16, 6), np.ones((4, 4, 4), np.uint8)):
        records = R.rects(V, True)
        verts, quads = VoxelVolume.meshFromFaces(records, merged=True)
        assert verts.dtype == np.int32 and quads.dtype == np.int64 and quads.shape == (records.shape[0], 4)
        assert len(np.unique(verts, axis=0)) == len(verts) and set(np.unique(quads)) == set(range(len(verts)))
        t = R.triangles(records).reshape(-1, 6, 3)
        c = 64 * verts[quads].astype(np.int64)
        u = R.unpack(records)
        for i in range(len(records)):
            assert {tuple(p) for p in c[i].tolist()} == {tuple(p) for p in t[i].tolist()} and len({tuple(p) for p in c[i].tolist()}) == 4
        axis, side = u[:, 3] >> 1, u[:, 3] & 1
        for k in range(4):
            turn = np.cross(c[:, (k + 1) % 4] - c[:, k], c[:, (k + 2) % 4] - c[:, (k + 1) % 4])
            assert np.array_equal(np.sign(turn[np.arange(len(u)), axis]), np.where(side == 1, 1, -1))
        # the default leaves the face mesh as it was: records read as faces have extent 1
        faces = F.faces(V, True)
        a, b = VoxelVolume.meshFromFaces(faces), VoxelVolume.meshFromFaces(faces, merged=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    verts, quads = VoxelVolume.meshFromFaces(R.rects(np.ones((4, 4, 4), np.uint8)), merged=True)
    assert len(verts) == 8 and len(quads) == 6
    path = tmp_path / "cube.obj"
    scenes.write_obj(str(path), verts, quads)
    assert len(path.read_text().splitlines()) == 14


def test_rect_refusals_need_no_gpu(built):
    """Every refusal decided before the first HIP call, with the return code and the WHOLE vrc_last_error() text as
    literals, as tests/test_volume_messages_host.py holds the other volume calls: NULL volume, unknown format or memory kind,
    NULL out with a capacity, a misaligned device buffer, NULL counts.  The handle is no volume at all, so a call that
    reached the device would fail in another way; nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    fake = (C.c_uint64 * 64)()
    pv = C.cast(fake, C.c_void_p)
    out = np.zeros(64, np.uint32)
    o = capi.ptr(out)
    total = C.c_uint64(7)
    cases = [((None, 1, 0, 0, 4, o, C.byref(total), 0, None), "null volume"),
             ((pv, 1, 2, 0, 4, o, C.byref(total), 0, None), "bad format 2"),
             ((pv, 1, -1, 0, 4, o, C.byref(total), 1, None), "bad format -1"),
             ((pv, 1, 0, 0, 4, o, C.byref(total), 2, None), "bad mem kind 2"),
             ((pv, 1, 1, 0, 4, o, C.byref(total), -1, None), "bad mem kind -1"),
             ((pv, 1, 0, 0, 4, None, C.byref(total), 0, None), "null buffer with capacity 4"),
             ((pv, 1, 1, 0, 5, None, C.byref(total), 1, None), "null buffer with capacity 5"),
             ((pv, 1, 0, 0, 4, C.c_void_p(0x1004), None, 1, None), "device buffer 0x1004 is not aligned to 16 bytes"),
             ((pv, 1, 1, 0, 4, C.c_void_p(0x1002), None, 1, None), "device buffer 0x1002 is not aligned to 4 bytes")]
    for args, text in cases:
        assert L.vrc_extract_rects(*args) == -1, text
        assert L.vrc_last_error() == b"vrc_extract_rects: " + text.encode()
    counts = np.zeros(6, np.uint64)
    assert L.vrc_rect_count(None, 1, capi.ptr(counts)) == -1 and L.vrc_last_error() == b"vrc_rect_count: null volume"
    assert L.vrc_rect_count(pv, 1, None) == -1 and L.vrc_last_error() == b"vrc_rect_count: null counts"
    assert total.value == 7 and not any(fake) and not out.any() and not counts.any()


def test_host_adapter_with_rects_compiles(built):
    """HipVoxelVolume::rectCount / surfaceRects / rectTriangles / extractRectsDevice / toObj(merged) in the header-only
    adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, void* dev, uint64_t* total_dev) {\n'
           '    const std::vector<uint64_t> counts = world.rectCount();\n'
           '    const std::vector<uint32_t> rects = world.surfaceRects(false, 3, 10);\n'
           '    const std::vector<int32_t> tris = world.rectTriangles();\n'
           '    world.extractRectsDevice(VRC_SURFACE_TRIANGLES, 0, 100, dev, total_dev);\n'
           '    world.extractRectsDevice(VRC_SURFACE_FACES, 0, 100, dev, nullptr, false, nullptr);\n'
           '    return counts[VRC_FACE_ZP] + rects.size() + tris.size() + world.toObj("world.obj", true, true) + world.toObj("open.obj", false);\n'
           '}\nint main(){ return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
    main = os.path.join(ROOT, "tests", "cpp", "voxel_rects_main.cpp")
    check_cpp_syntax(main, strict=True)
