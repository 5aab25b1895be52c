"""Merged-rectangle extraction on the GPU (vrc_rect_count / vrc_extract_rects, VoxelVolume.rectCount /
surfaceRects / rectTriangles / extractRectsDevice / toMesh(merged=True)).  The expected rectangles are the numpy model's
(tests/rect_model.py, held against a per-cell restatement of the definition in tests/test_volume_rects_host.py); every
comparison is exact and in the canonical order (d, c_a, s0, r0).  Shapes are the smallest at which the kernels take another
path: 4^3 and 8^3 (a row is shorter than a word, gathered bit by bit), 32^3 (a row is one word), 64^3 (runs cross a word
boundary, 192 workgroups), 128^3 (4 words per row, 1536 workgroup slots: the scan's second step; dense, more records than
one internal window of the host form), and 1024^3 once for the 64-bit indexing and the extreme of the packing."""
import ctypes as C
import functools

import numpy as np
import pytest

import rect_model as R
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def random_field(depth, density):
    S = 1 << depth
    V = (np.random.default_rng(2000 * depth + int(100 * density)).random((S, S, S)) < density).astype(np.uint8)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def model_rects(depth, density, closed):
    r = R.rects(random_field(depth, density), closed)
    r.setflags(write=False)
    return r


def block_bytes(depth):
    """the documented size of the rectangle calls' block: offsets and totals, then the two row fields"""
    S = 1 << depth
    w = max(1, S // 32)
    lanes = 6 * S * S * w
    return 8 * ((lanes + 255) // 256 + 7) + 8 * S * S * w


def lane_of(records, S):
    """the lane (d, c_a, c_s, word of the row) that emits each record"""
    u = R.unpack(records)
    rows = np.arange(u.shape[0])
    a = u[:, 3] >> 1
    w = max(1, S // 32)
    return ((u[:, 3] * S + u[rows, a]) * S + u[rows, np.asarray(R.STACK)[a]]) * w + u[rows, np.asarray(R.RUN)[a]] // 32


def check_volume(volume, V, what, rects_of=None):
    """counts, R by capacity 0, records and triangles of `volume`, closed and open, against the model of the dense field V"""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    for closed in (True, False):
        want = rects_of(closed) if rects_of else R.rects(V, closed)
        counts = volume.rectCount(closed)
        assert counts.dtype == np.uint64 and np.array_equal(counts, R.direction_counts(want)), (what, closed, counts)
        total = C.c_uint64()
        assert L.vrc_extract_rects(volume._h, int(closed), 0, 0, 0, None, C.byref(total), 0, None) == 0
        assert total.value == int(counts.sum()) == want.shape[0], (what, closed)
        got = volume.surfaceRects(closed)
        assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), (what, closed)
        tris = volume.rectTriangles(closed)
        assert tris.dtype == np.int32 and np.array_equal(tris, R.triangles(want)), (what, closed)


# ---- random fields at every depth with a path of its own ------------------------------------------------------------

@pytest.mark.parametrize("depth,density", [(2, 0.5), (3, 0.5), (5, 0.5), (5, 0.9), (6, 0.5), (7, 0.02), (7, 0.5)])
def test_random_fields(built, depth, density):
    volume = volume_of(random_field(depth, density))
    before = volume.editScratchBytes()                      # setVoxels' staging; nothing of the rectangle calls yet
    volume.rectCount()
    assert volume.editScratchBytes() == before + block_bytes(depth)
    check_volume(volume, None, (depth, density), lambda closed: model_rects(depth, density, closed))
    if (depth, density) == (7, 0.5):
        # more records than one internal window of 2^20, stitched inside one call of the C ABI
        import cpuvoxelraycaster_amd as vrc
        want = model_rects(depth, density, True)
        T = want.shape[0]
        assert T > (1 << 20) and 6 * 128 * 128 * 4 // 256 > 1024      # and the scan of the slots takes a second step
        out = np.zeros((2 * T, 9), np.int32)
        total = C.c_uint64()
        vrc.capi.check(vrc.capi.load().vrc_extract_rects(volume._h, 1, vrc.capi.VRC_SURFACE_TRIANGLES, 0, 1 << 40, vrc.capi.ptr(out),
                                                               C.byref(total), 0, None))
        assert total.value == T and np.array_equal(out, R.triangles(want))
    volume.close()


def constructed_fields(S):
    """each pair in consecutive rows, scaled to S with h = S / 2 (at 64^3 h is the word boundary): on the +y faces of
    one-voxel-thick sheets at y = 7 the rows stack along x and run along z; at z = 20 (the z faces) they stack along x and
    run along y"""
    h = S // 2
    assert S >= 32
    V = np.zeros((S, S, S), np.uint8)
    V[3, 7, 0:h], V[4, 7, 0:h + 1] = 1, 1                   # at 64^3 the identical-run test looks one bit into the next word
    V[10, 7, 1:h + 8], V[11, 7, 0:h + 8] = 1, 1
    V[20, 7, 5:20], V[21, 7, 5:20], V[22, 7, 5:21] = 1, 1, 1      # heights 2 and 1
    V[28, 7, :], V[29, 7, :] = 1, 1                         # a full-length row above one with a hole
    V[29, 7, h + 5] = 0
    V[14, 0:h, 20], V[15, 0:h + 1, 20] = 1, 1
    V[24, :, 20], V[25, :, 20] = 1, 1
    V[25, h, 20] = 0
    return V


@pytest.mark.parametrize("depth", [5, 6])
def test_constructed_fields(built, depth):
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    empty = vrc.VoxelVolume(depth)
    check_volume(empty, np.zeros((S, S, S), np.uint8), "empty")
    assert empty.surfaceRects().shape == (0, 4) and empty.rectTriangles().shape == (0, 9)
    empty.close()
    full = vrc.VoxelVolume(depth)
    full.fillBoxes([[0, 0, 0, S, S, S]])
    check_volume(full, np.ones((S, S, S), np.uint8), "full")
    u = vrc.VoxelVolume.unpackRects(full.surfaceRects())
    assert u.shape == (6, 6) and np.all(u[:, 4:] == S) and full.rectCount(False).sum() == 0
    full.close()
    board = (np.indices((S, S, S)).sum(axis=0) & 1).astype(np.uint8)
    volume = volume_of(board)
    check_volume(volume, board, "checkerboard")
    assert volume.rectCount().sum() == volume.surfaceCount().sum() == 6 * board.sum()
    volume.close()
    corners = np.zeros((S, S, S), np.uint8)
    for x in (0, S - 1):
        for y in (0, S - 1):
            for z in (0, S - 1):
                corners[x, y, z] = 1
    volume = volume_of(corners)
    check_volume(volume, corners, "corners")
    assert volume.rectCount(True).sum() == 48 and volume.rectCount(False).sum() == 24
    volume.close()
    for axis in range(3):
        for side in (0, 1):
            lo, hi = [0, 0, 0], [S, S, S]
            lo[axis], hi[axis] = (S - 1, S) if side else (0, 1)
            V = np.zeros((S, S, S), np.uint8)
            V[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
            volume = vrc.VoxelVolume(depth)
            volume.fillBoxes([lo + hi])
            check_volume(volume, V, ("slab", axis, side))
            assert volume.rectCount(True).sum() == 6 and volume.rectCount(False).sum() == 1
            volume.close()
    V = constructed_fields(S)
    volume = volume_of(V)
    check_volume(volume, V, "constructed")
    up = vrc.VoxelVolume.unpackRects(volume.surfaceRects(False))
    up = up[(up[:, 3] == 3) & (up[:, 1] == 7)]
    h = S // 2
    assert up.tolist() == [[3, 7, 0, 3, h, 1], [4, 7, 0, 3, h + 1, 1], [10, 7, 1, 3, h + 7, 1], [11, 7, 0, 3, h + 8, 1], [20, 7, 5, 3, 15, 2],
                           [22, 7, 5, 3, 16, 1], [28, 7, 0, 3, S, 1], [29, 7, 0, 3, h + 5, 1], [29, 7, h + 6, 3, h - 6, 1]]
    down = vrc.VoxelVolume.unpackRects(volume.surfaceRects(False))
    down = down[(down[:, 3] == 5) & (down[:, 2] == 20) & np.isin(down[:, 0], (14, 15, 24, 25))]
    assert down.tolist() == [[14, 0, 20, 5, h, 1], [15, 0, 20, 5, h + 1, 1], [24, 0, 20, 5, S, 1], [25, 0, 20, 5, h, 1], [25, h + 1, 20, 5, h - 1, 1]]
    volume.close()


# ---- windows ----------------------------------------------------------------------------------------------------------

def test_windows(built):
    """Window edges inside one row's rectangles, on a row boundary, on a workgroup boundary (256 lanes) and just before it;
    capacities 1, 7, T - 1, T, T + 5; a sentinel behind what is written stays intact."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, density = 6, 0.5
    S = 1 << depth
    want = model_rects(depth, density, True)
    want_tris = R.triangles(want)
    T = want.shape[0]
    lane = lane_of(want, S)
    assert np.all(np.diff(lane) >= 0)
    row = lane // (S // 32)
    starts = np.flatnonzero(np.diff(row, prepend=-1) != 0)              # the first rectangle of every row that has one
    sizes = np.diff(np.append(starts, T))
    k = int(np.flatnonzero(sizes >= 3)[5])
    inside, row_edge = int(starts[k]) + 1, int(starts[k + 1])
    group_edge = int(np.searchsorted(lane // 256, 3))                   # the first rectangle of the fourth workgroup
    assert 0 < inside < row_edge < T and 0 < group_edge < T and lane[group_edge - 1] // 256 < 3 <= lane[group_edge] // 256
    volume = volume_of(random_field(depth, density))
    L = vrc.capi.load()

    for fmt, per, rows, expect in ((vrc.capi.VRC_SURFACE_FACES, 4, 1, want), (vrc.capi.VRC_SURFACE_TRIANGLES, 18, 2, want_tris)):
        dtype = np.uint32 if fmt == vrc.capi.VRC_SURFACE_FACES else np.int32
        for first in (0, inside, row_edge, group_edge, group_edge - 3, T - 3, T, T + 9):
            for cap in (1, 7, T - 1, T, T + 5):
                n = max(0, min(cap, T - first))
                buf = np.full((min(cap, T + 5) + 4, per), SENTINEL, dtype)
                total = C.c_uint64()
                vrc.capi.check(L.vrc_extract_rects(volume._h, 1, fmt, first, cap, vrc.capi.ptr(buf), C.byref(total), 0, None))
                assert total.value == T
                assert np.array_equal(buf[:n].reshape(-1, per // rows), expect[rows * first:rows * (first + n)]), (fmt, first, cap)
                assert np.all(buf[n:] == SENTINEL), (fmt, first, cap)
                dev = torch.full((min(cap, T + 5) + 4, per), SENTINEL, dtype=torch.int32, device="cuda")
                dev_total = torch.zeros(1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                volume.extractRectsDevice(fmt, first, cap, dev.data_ptr(), dev_total.data_ptr())
                torch.cuda.synchronize()
                got = dev.cpu().numpy().view(dtype)
                assert int(dev_total.item()) == T
                assert np.array_equal(got[:n].reshape(-1, per // rows), expect[rows * first:rows * (first + n)]), (fmt, first, cap, "device")
                assert np.all(got[n:] == SENTINEL), (fmt, first, cap, "device")
    # consecutive windows give the full list
    edges = [0, inside, row_edge, group_edge - 3, group_edge, group_edge + 1000, T]
    parts = [volume.surfaceRects(True, a, b - a) for a, b in zip(edges[:-1], edges[1:])]
    assert np.array_equal(np.concatenate(parts), want)
    parts = [volume.rectTriangles(True, a, b - a) for a, b in zip(edges[:-1], edges[1:])]
    assert np.array_equal(np.concatenate(parts), want_tris)
    # capacity 0 / out NULL gives T, in device memory too
    total = C.c_uint64()
    vrc.capi.check(L.vrc_extract_rects(volume._h, 1, 0, 5, 0, None, C.byref(total), 0, None))
    assert total.value == T
    dev_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    volume.extractRectsDevice(vrc.capi.VRC_SURFACE_FACES, 0, 0, None, dev_total.data_ptr())
    torch.cuda.synchronize()
    assert int(dev_total.item()) == T
    assert volume.surfaceRects(True, T).shape == (0, 4) and volume.surfaceRects(True, T + 100, 10).shape == (0, 4)
    # a misaligned device buffer is refused, not written
    dev = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert L.vrc_extract_rects(volume._h, 1, 0, 0, 2, C.c_void_p(dev.data_ptr() + 4), None, 1, None) == -1
    assert b"aligned" in L.vrc_last_error()
    assert L.vrc_extract_rects(volume._h, 1, 1, 0, 2, C.c_void_p(dev.data_ptr() + 2), None, 1, None) == -1
    torch.cuda.synchronize()
    assert not dev.cpu().numpy().any()
    # triangles at an address that is 4- but not 8-byte aligned take the narrow stores
    dev = torch.full((1 + 18 * 10 + 3,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    volume.extractRectsDevice(vrc.capi.VRC_SURFACE_TRIANGLES, inside, 10, dev.data_ptr() + 4, None)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(got[1:181].reshape(-1, 9), want_tris[2 * inside:2 * inside + 20]) and np.all(got[181:] == SENTINEL) and got[0] == SENTINEL
    volume.close()


# ---- the round trip ---------------------------------------------------------------------------------------------------

def test_round_trip_on_the_device(built):
    """extractRectsDevice triangles, then xorMesh into a fresh volume on the same stream, gives the source: for the random
    64^3 field and a voxelised icosphere; a second xorMesh of them empties the volume again."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth = 6
    ball = vrc.VoxelVolume(depth)
    verts, faces = vrc.icosphere(2)
    ball.voxelizeMesh(verts, faces, 24.3, (31.2, 30.7, 33.4))
    assert ball.solidCount() > 40000
    for volume in (volume_of(random_field(depth, 0.5)), ball):
        V = volume.download()
        T = int(volume.rectCount().sum())
        assert T <= int(volume.surfaceCount().sum())
        tris = torch.zeros((2 * T, 9), dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        back = vrc.VoxelVolume(depth)
        with Stream() as stream:
            volume.extractRectsDevice(vrc.capi.VRC_SURFACE_TRIANGLES, 0, T, tris.data_ptr(), total.data_ptr(), True, stream)
            back.xorMesh((2 * T, tris.data_ptr()), device=True, stream=stream)
            assert np.array_equal(back.download(), V)
            assert int(total.item()) == T
            back.xorMesh((2 * T, tris.data_ptr()), device=True, stream=stream)
            assert back.solidCount() == 0
        back.close()
        volume.close()


def test_ordered_behind_device_edits(built):
    """fillSpheresDevice on a stream, then extractRectsDevice on the same stream: the extraction sees the spheres; the
    synchronous rectCount afterwards, on the NULL stream, agrees."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 6, 64
    spheres = np.array([[20, 20, 20, 9], [40, 44, 30, 12], [62, 3, 60, 7]], np.int32)
    g = np.indices((S, S, S)).astype(np.int64)
    V = np.zeros((S, S, S), np.uint8)
    for cx, cy, cz, r in spheres.tolist():
        V |= ((g[0] - cx) ** 2 + (g[1] - cy) ** 2 + (g[2] - cz) ** 2 <= r * r).astype(np.uint8)
    want = R.rects(V, True)
    t_spheres = torch.from_numpy(spheres).cuda()
    out = torch.zeros((want.shape[0] + 8, 4), dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    volume = vrc.VoxelVolume(depth)
    with Stream() as stream:
        volume.fillSpheresDevice(len(spheres), t_spheres.data_ptr(), True, stream)
        volume.extractRectsDevice(vrc.capi.VRC_SURFACE_FACES, 0, want.shape[0] + 8, out.data_ptr(), total.data_ptr(), True, stream)
    torch.cuda.synchronize()
    assert int(total.item()) == want.shape[0]
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:want.shape[0]], want) and not got[want.shape[0]:].any()
    assert np.array_equal(volume.rectCount(), R.direction_counts(want))
    volume.close()


def test_scratch_is_allocated_once_and_only_by_these_calls(built):
    import cpuvoxelraycaster_amd as vrc
    depth = 6
    V = random_field(depth, 0.5)
    volume = volume_of(V)
    before = volume.editScratchBytes()                      # setVoxels' staging alone
    other = volume_of(V)                                    # never makes a rectangle call: what it reported before
    assert other.editScratchBytes() == before
    other.surfaceCount()
    assert other.editScratchBytes() == before + 8 * (8 ** depth // 32 // 256 + 7)        # the surface calls' offsets block
    total = C.c_uint64()
    vrc.capi.check(vrc.capi.load().vrc_extract_rects(volume._h, 1, 0, 0, 0, None, C.byref(total), 0, None))
    after = volume.editScratchBytes()
    assert after == before + block_bytes(depth) == before + 8 * (192 + 7) + 8 * 64 * 64 * 2
    for i in range(10):
        assert volume.surfaceRects(i % 2 == 0, 1000 * i, 500).shape == (500, 4)           # 500 records fit the staging block
        volume.rectCount(i % 2 == 1)
    assert volume.editScratchBytes() == after
    volume.close()
    other.close()


def test_merged_mesh_of_a_volume(built):
    import cpuvoxelraycaster_amd as vrc
    V = random_field(5, 0.9)
    volume = volume_of(V)
    verts, quads = volume.toMesh(merged=True)
    want_verts, want_quads = vrc.VoxelVolume.meshFromFaces(R.rects(V, True), merged=True)
    assert np.array_equal(verts, want_verts) and np.array_equal(quads, want_quads)
    assert quads.shape[0] < volume.toMesh()[1].shape[0]
    volume.close()


# ---- 64-bit indexing and the extreme of the packing ---------------------------------------------------------------------

def test_depth_10(built):
    """1024^3, once: three small boxes at the origin corner and three at the far corner, each group modelled in a 32^3 field
    aligned to its corner with a margin to the field's other sides, translated and ordered by (d, c_a, s0, r0); then the
    whole volume filled: six records with nr = ns = 1024, the extreme of the packing and of one lane's row walk."""
    import cpuvoxelraycaster_amd as vrc
    depth, S, m = 10, 1024, 32
    near = [[0, 0, 0, 3, 2, 5], [0, 6, 0, 1, 9, 1], [7, 0, 9, 12, 4, 11]]
    far = [[m - 3, m - 2, m - 5, m, m, m], [m - 1, m - 9, m - 1, m, m - 6, m], [m - 12, m - 4, m - 11, m - 7, m, m - 9]]
    volume = vrc.VoxelVolume(depth)
    shift = S - m
    volume.fillBoxes(near + [[c + shift for c in box] for box in far])
    before, most = volume.editScratchBytes(), 0
    for closed in (True, False):
        parts = []
        for boxes, off in ((near, 0), (far, shift)):
            V = np.zeros((m, m, m), np.uint8)
            for x0, y0, z0, x1, y1, z1 in boxes:
                V[x0:x1, y0:y1, z0:z1] = 1
            assert not V[m // 2].any() and not V[:, m // 2].any() and not V[:, :, m // 2].any()      # the margin
            r = R.rects(V, closed).astype(np.int64)
            r[:, :3] += off
            parts.append(r)
        want = R.ordered(np.concatenate(parts))
        most = max(most, want.shape[0])
        assert np.array_equal(volume.rectCount(closed), R.direction_counts(want)), closed
        got = volume.surfaceRects(closed)
        assert np.array_equal(got, want), closed
        assert np.array_equal(volume.rectTriangles(closed), R.triangles(want)), closed
        assert got[:, :3].max() == S - 1 and got[:, :3].min() == 0
    assert volume.editScratchBytes() == max(before, 72 * most) + block_bytes(depth)       # staging of the largest call + the block
    # a window that starts in the far group: the workgroups before it leave after reading their offsets
    k = int(np.argmax(want[:, 0] >= shift))
    assert 0 < k < want.shape[0] - 7 and np.array_equal(volume.surfaceRects(False, k, 7), want[k:k + 7])
    volume.fillBoxes([[0, 0, 0, S, S, S]])
    assert np.array_equal(volume.rectCount(True), np.ones(6, np.uint64)) and volume.rectCount(False).sum() == 0
    got = volume.surfaceRects(True)
    far_side = [[0, 0, 0], [S - 1, 0, 0], [0, 0, 0], [0, S - 1, 0], [0, 0, 0], [0, 0, S - 1]]
    assert np.array_equal(got, R.pack(far_side, np.arange(6), np.full(6, S), np.full(6, S)))
    assert np.array_equal(volume.rectTriangles(True), R.triangles(got))
    volume.close()
