"""Surface extraction on the GPU (vrc_volume_surface_count / vrc_volume_extract_surface, VoxelVolume.surfaceCount /
surfaceFaces / surfaceTriangles / extractSurfaceDevice / toMesh).  The expected faces are the numpy model's
(tests/surface_model.py, held against a per-voxel loop and the voxeliser's model in tests/test_volume_surface_host.py);
every comparison is exact and in the canonical order.  Shapes are the smallest at which the kernels take another path:
4^3 (two words, a word straddles two brick rows), 8^3 (a column is one word), 32^3 (4 workgroups of words), 64^3 (32),
128^3 (256 workgroups and, dense, more faces than one internal window of the host form), and 1024^3 once for the 64-bit
indexing."""
import ctypes as C
import functools

import numpy as np
import pytest

import surface_model as F
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def random_field(depth, density):
    S = 1 << depth
    V = (np.random.default_rng(1000 * depth + int(100 * density)).random((S, S, S)) < density).astype(np.uint8)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def model_faces(depth, density, closed):
    f = F.faces(random_field(depth, density), closed)
    f.setflags(write=False)
    return f


def offsets_bytes(depth):
    """the documented size of the surface calls' offsets block"""
    words = 8 ** depth // 32
    return 8 * ((words + 255) // 256 + 7)


def check_volume(volume, V, what, faces_of=None):
    """counts, faces and triangles of `volume`, closed and open, against the model of the dense field V"""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    for closed in (True, False):
        want = faces_of(closed) if faces_of else F.faces(V, closed)
        counts = volume.surfaceCount(closed)
        assert counts.dtype == np.uint64 and np.array_equal(counts, F.direction_counts(want)), (what, closed, counts)
        total = C.c_uint64()
        assert L.vrc_volume_extract_surface(volume._h, int(closed), 0, 0, 0, None, C.byref(total), 0, None) == 0
        assert total.value == int(counts.sum()) == want.shape[0], (what, closed)
        got = volume.surfaceFaces(closed)
        assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), (what, closed)
        tris = volume.surfaceTriangles(closed)
        assert tris.dtype == np.int32 and np.array_equal(tris, F.triangles(want)), (what, closed)


# ---- random fields at every depth with a path of its own ------------------------------------------------------------

@pytest.mark.parametrize("depth,density", [(2, 0.5), (3, 0.5), (5, 0.5), (6, 0.5), (7, 0.02), (7, 0.5)])
def test_random_fields(built, depth, density):
    volume = volume_of(random_field(depth, density))
    before = volume.editScratchBytes()                      # setVoxels' staging; nothing of the surface calls yet
    volume.surfaceCount()
    assert volume.editScratchBytes() == before + offsets_bytes(depth)
    check_volume(volume, None, (depth, density), lambda closed: model_faces(depth, density, closed))
    volume.close()


@pytest.mark.parametrize("depth", [2, 3, 5])
def test_special_fields(built, depth):
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    empty = vrc.VoxelVolume(depth)
    check_volume(empty, np.zeros((S, S, S), np.uint8), "empty")
    assert empty.surfaceFaces().shape == (0, 4) and empty.surfaceTriangles().shape == (0, 9)
    empty.close()
    full = vrc.VoxelVolume(depth)
    full.fillBoxes([[0, 0, 0, S, S, S]])
    check_volume(full, np.ones((S, S, S), np.uint8), "full")
    assert full.surfaceCount(False).sum() == 0 and np.array_equal(full.surfaceCount(True), np.full(6, S * S))
    full.close()
    board = (np.indices((S, S, S)).sum(axis=0) & 1).astype(np.uint8)
    volume = volume_of(board)
    check_volume(volume, board, "checkerboard")
    assert volume.surfaceCount().sum() == 6 * board.sum()
    volume.close()
    for x in (0, S - 1):
        for y in (0, S - 1):
            for z in (0, S - 1):
                V = np.zeros((S, S, S), np.uint8)
                V[x, y, z] = 1
                volume = volume_of(V)
                check_volume(volume, V, ("corner", x, y, z))
                assert volume.surfaceCount(True).sum() == 6 and volume.surfaceCount(False).sum() == 3
                volume.close()
    # a one-voxel-thick slab on each wall: where closed and open differ
    for axis in range(3):
        for side in (0, 1):
            lo, hi = [0, 0, 0], [S, S, S]
            lo[axis], hi[axis] = (S - 1, S) if side else (0, 1)
            V = np.zeros((S, S, S), np.uint8)
            V[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
            volume = vrc.VoxelVolume(depth)
            volume.fillBoxes([lo + hi])
            check_volume(volume, V, ("slab", axis, side))
            want_open = np.zeros(6, np.uint64)
            want_open[2 * axis + (1 - side)] = S * S
            assert np.array_equal(volume.surfaceCount(False), want_open)
            assert volume.surfaceCount(True).sum() == 2 * S * S + 4 * S
            volume.close()


# ---- windows ----------------------------------------------------------------------------------------------------------

def test_windows(built):
    """Window edges inside one word's faces of one direction, between two directions of a word, on a word boundary and on
    a workgroup boundary (256 words); capacities 1, 7, T - 1, T, T + 5; a sentinel behind what is written stays intact."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, density = 6, 0.5
    S = 1 << depth
    want = model_faces(depth, density, True)
    want_tris = F.triangles(want)
    T = want.shape[0]
    per_word = F.word_direction_counts(want, S)
    start = np.concatenate([[0], np.cumsum(per_word.reshape(-1))]).reshape(-1)      # first face of (word, direction)
    w = int(np.flatnonzero((per_word[:, 0] >= 3) & (per_word[:, 1] >= 1))[1])
    assert per_word[w, 0] >= 3 and w > 0
    inside = int(start[6 * w]) + 1                          # the second face of direction 0 of word w
    between = int(start[6 * w + 1])                         # its first face of direction 1
    word_edge = int(start[6 * (w + 1)])
    group_edge = int(start[6 * 256 * 3])                    # the first face of the fourth workgroup
    assert 0 < inside < between <= word_edge and 0 < group_edge < T
    volume = volume_of(random_field(depth, density))
    L = vrc.capi.load()

    for fmt, per, rows, expect in ((vrc.capi.VRC_SURFACE_FACES, 4, 1, want), (vrc.capi.VRC_SURFACE_TRIANGLES, 18, 2, want_tris)):
        dtype = np.uint32 if fmt == vrc.capi.VRC_SURFACE_FACES else np.int32
        for first in (0, inside, between, word_edge, group_edge, group_edge - 3, T - 3, T, T + 9):
            for cap in (1, 7, T - 1, T, T + 5):
                n = max(0, min(cap, T - first))
                if cap >= T - 1 and first not in (0, inside, group_edge):
                    continue                                # the large capacities with three of the starts: enough
                # host memory: a buffer longer than the window, filled with a sentinel
                buf = np.full((min(cap, T + 5) + 4, per), 0x5A5A5A5A, dtype)
                total = C.c_uint64()
                vrc.capi.check(L.vrc_volume_extract_surface(volume._h, 1, fmt, first, cap, vrc.capi.ptr(buf), C.byref(total), 0, None))
                assert total.value == T
                assert np.array_equal(buf[:n].reshape(-1, per // rows), expect[rows * first:rows * (first + n)]), (fmt, first, cap)
                assert np.all(buf[n:] == 0x5A5A5A5A), (fmt, first, cap)
                # device memory
                dev = torch.full((min(cap, T + 5) + 4, per), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                dev_total = torch.zeros(1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                volume.extractSurfaceDevice(fmt, first, cap, dev.data_ptr(), dev_total.data_ptr())
                torch.cuda.synchronize()
                got = dev.cpu().numpy().view(dtype)
                assert int(dev_total.item()) == T
                assert np.array_equal(got[:n].reshape(-1, per // rows), expect[rows * first:rows * (first + n)]), (fmt, first, cap, "device")
                assert np.all(got[n:] == 0x5A5A5A5A), (fmt, first, cap, "device")
    # consecutive windows give the full list
    edges = [0, inside, between, word_edge, group_edge - 3, group_edge, group_edge + 1000, T]
    parts = [volume.surfaceFaces(True, a, b - a) for a, b in zip(edges[:-1], edges[1:])]
    assert np.array_equal(np.concatenate(parts), want)
    parts = [volume.surfaceTriangles(True, a, b - a) for a, b in zip(edges[:-1], edges[1:])]
    assert np.array_equal(np.concatenate(parts), want_tris)
    # capacity 0 / out NULL gives T, in device memory too
    total = C.c_uint64()
    vrc.capi.check(L.vrc_volume_extract_surface(volume._h, 1, 0, 5, 0, None, C.byref(total), 0, None))
    assert total.value == T
    dev_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    volume.extractSurfaceDevice(vrc.capi.VRC_SURFACE_FACES, 0, 0, None, dev_total.data_ptr())
    torch.cuda.synchronize()
    assert int(dev_total.item()) == T
    assert volume.surfaceFaces(True, T).shape == (0, 4) and volume.surfaceFaces(True, T + 100, 10).shape == (0, 4)
    # a misaligned device buffer is refused, not written
    dev = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert L.vrc_volume_extract_surface(volume._h, 1, 0, 0, 2, C.c_void_p(dev.data_ptr() + 4), None, 1, None) == -1
    assert b"aligned" in L.vrc_last_error()
    # triangles at an address that is 4- but not 8-byte aligned take the narrow stores
    dev = torch.full((1 + 18 * 10 + 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    volume.extractSurfaceDevice(vrc.capi.VRC_SURFACE_TRIANGLES, inside, 10, dev.data_ptr() + 4, None)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(got[1:181].reshape(-1, 9), want_tris[2 * inside:2 * inside + 20]) and np.all(got[181:] == 0x5A5A5A5A) and got[0] == 0x5A5A5A5A
    volume.close()


# ---- the round trip ---------------------------------------------------------------------------------------------------

def test_round_trip_on_the_device(built):
    """surfaceTriangles of V voxelised into a fresh volume gives V: for the random 64^3 field and a voxelised icosphere;
    and with the triangles never leaving the device, where a second xorMesh of them empties the volume again."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    ball = vrc.VoxelVolume(depth)
    verts, faces = vrc.icosphere(2)
    ball.voxelizeMesh(verts, faces, 24.3, (31.2, 30.7, 33.4))
    assert ball.solidCount() > 40000
    for volume in (volume_of(random_field(depth, 0.5)), ball):
        V = volume.download()
        back = vrc.VoxelVolume(depth)
        back.xorMesh(volume.surfaceTriangles())
        assert np.array_equal(back.download(), V)
        back.close()
        # on the device, on one stream
        T = int(volume.surfaceCount().sum())
        tris = torch.zeros((2 * T, 9), dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        back = vrc.VoxelVolume(depth)
        with Stream() as stream:
            volume.extractSurfaceDevice(vrc.capi.VRC_SURFACE_TRIANGLES, 0, T, tris.data_ptr(), total.data_ptr(), True, stream)
            back.xorMesh((2 * T, tris.data_ptr()), device=True, stream=stream)
            assert np.array_equal(back.download(), V)
            assert int(total.item()) == T
            back.xorMesh((2 * T, tris.data_ptr()), device=True, stream=stream)
            assert back.solidCount() == 0
        back.close()
        volume.close()


def test_ordered_behind_device_edits(built):
    """fillSpheresDevice on a stream, then extractSurfaceDevice on the same stream: the extraction sees the spheres, and
    the total arrives in the device word."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    spheres = np.array([[20, 20, 20, 9], [40, 44, 30, 12], [62, 3, 60, 7]], np.int32)
    g = np.indices((S, S, S)).astype(np.int64)
    V = np.zeros((S, S, S), np.uint8)
    for cx, cy, cz, r in spheres.tolist():
        V |= ((g[0] - cx) ** 2 + (g[1] - cy) ** 2 + (g[2] - cz) ** 2 <= r * r).astype(np.uint8)
    want = F.faces(V, True)
    t_spheres = torch.from_numpy(spheres).cuda()
    out = torch.zeros((want.shape[0] + 8, 4), dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    volume = vrc.VoxelVolume(depth)
    with Stream() as stream:
        volume.fillSpheresDevice(len(spheres), t_spheres.data_ptr(), True, stream)
        volume.extractSurfaceDevice(vrc.capi.VRC_SURFACE_FACES, 0, want.shape[0] + 8, out.data_ptr(), total.data_ptr(), True, stream)
    torch.cuda.synchronize()
    assert int(total.item()) == want.shape[0]
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:want.shape[0]], want) and not got[want.shape[0]:].any()
    # and the synchronous count, on the NULL stream, waits for an extraction still in flight on another
    assert np.array_equal(volume.surfaceCount(), F.direction_counts(want))
    volume.close()


def test_host_form_is_stitched_and_scratch_is_bounded(built):
    """capacity=None on the dense 128^3 field: more faces than one internal window of 2^20, in one call of the C ABI too.
    The staging block stays at 2^20 records, the offsets block is 8 * (ceil(words / 256) + 7) bytes, and ten more
    extractions grow nothing."""
    import cpuvoxelraycaster_amd as vrc
    depth, density = 7, 0.5
    want = model_faces(depth, density, True)
    T = want.shape[0]
    assert T > 2 * (1 << 20)
    volume = volume_of(random_field(depth, density))
    assert volume.editScratchBytes() < 72 << 20              # setVoxels' staging
    # one call of the C ABI for everything: stitched inside the library
    out = np.zeros((2 * T, 9), np.int32)
    total = C.c_uint64()
    vrc.capi.check(vrc.capi.load().vrc_volume_extract_surface(volume._h, 1, vrc.capi.VRC_SURFACE_TRIANGLES, 0, 1 << 40, vrc.capi.ptr(out),
                                                             C.byref(total), 0, None))
    assert total.value == T and np.array_equal(out, F.triangles(want))
    offsets = offsets_bytes(depth)
    assert offsets <= 8 ** depth // 8 // 64                                       # at most 1/64 of the occupancy
    assert volume.editScratchBytes() == 72 * (1 << 20) + offsets
    assert np.array_equal(volume.surfaceFaces(True), want)                        # stitched by the Python form
    after = volume.editScratchBytes()
    for i in range(10):
        assert volume.surfaceTriangles(i % 2 == 0, 1000 * i, 5000).shape == (10000, 9)
    volume.surfaceCount()
    assert volume.editScratchBytes() == after == 72 * (1 << 20) + offsets
    volume.close()


def test_quad_mesh_of_a_volume(built):
    import cpuvoxelraycaster_amd as vrc
    V = random_field(5, 0.5)
    volume = volume_of(V)
    verts, quads = volume.toMesh()
    want_verts, want_quads = vrc.VoxelVolume.meshFromFaces(F.faces(V, True))
    assert np.array_equal(verts, want_verts) and np.array_equal(quads, want_quads)
    assert volume.toMesh(False)[1].shape[0] == F.faces(V, False).shape[0]
    volume.close()


# ---- 64-bit indexing --------------------------------------------------------------------------------------------------

def test_depth_10_corners(built):
    """1024^3, once: three small boxes at the origin corner and three at the far corner (coordinates up to 1023, word
    indices up to 2^25 - 1, the last workgroup of 131072), each group modelled in a 32^3 field aligned to its corner with
    a margin to the field's other sides, translated, and ordered with the model's key function at S = 1024.  This checks
    the 64-bit and last-word indexing; a total beyond 2^32 faces itself is NOT tested, because no entry point can fill
    such a field within a few seconds."""
    import cpuvoxelraycaster_amd as vrc
    depth, S, m = 10, 1024, 32
    near = [[0, 0, 0, 3, 2, 5], [0, 6, 0, 1, 9, 1], [7, 0, 9, 12, 4, 11]]
    far = [[m - 3, m - 2, m - 5, m, m, m], [m - 1, m - 9, m - 1, m, m - 6, m], [m - 12, m - 4, m - 11, m - 7, m, m - 9]]
    volume = vrc.VoxelVolume(depth)
    shift = S - m
    volume.fillBoxes(near + [[c + shift for c in box] for box in far])
    most = 0
    for closed in (True, False):
        parts = []
        for boxes, off in ((near, 0), (far, shift)):
            V = np.zeros((m, m, m), np.uint8)
            for x0, y0, z0, x1, y1, z1 in boxes:
                V[x0:x1, y0:y1, z0:z1] = 1
            assert not V[m // 2].any() and not V[:, m // 2].any() and not V[:, :, m // 2].any()      # the margin
            f = F.faces(V, closed).astype(np.int64)
            f[:, :3] += off
            parts.append(f)
        want = F.ordered(np.concatenate(parts), S)
        most = max(most, want.shape[0])
        assert np.array_equal(volume.surfaceCount(closed), F.direction_counts(want)), closed
        got = volume.surfaceFaces(closed)
        assert np.array_equal(got, want), closed
        assert np.array_equal(volume.surfaceTriangles(closed), F.triangles(want)), closed
        assert got[:, :3].max() == S - 1 and got[:, :3].min() == 0
    # a window that starts in the far group: the workgroups before it leave after reading their offsets
    k = int(np.argmax(want[:, 0] >= shift))
    assert 0 < k < want.shape[0] and np.array_equal(volume.surfaceFaces(False, k, 7), want[k:k + 7])
    assert offsets_bytes(depth) == 8 * (131072 + 7) <= 8 ** depth // 8 // 64
    assert volume.editScratchBytes() == max(72 * most, 24 * 6) + offsets_bytes(depth)      # staging of the largest call + the offsets
    volume.close()
