"""Surface extraction on the GPU (csrc/vrc_surface.hip) at the depths tests/test_gpu_volume_surface.py leaves out: 4 (16^3:
128 words, half a workgroup), 8 (256^3: 2048 workgroup slots, the first depth at which the scan of the slots takes a second
step with faces spread over all of them) and 9 (512^3: 16 384 slots, boxes only).  Every comparison is exact and in the
canonical order, against tests/surface_model.py."""
import ctypes as C

import numpy as np
import pytest

import surface_model as F
from large_volume_cases import SCAN_GROUP, scan_steps
from test_gpu_volume_surface import check_volume, offsets_bytes
from volume_support import volume_of

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


def test_depth_4(built):
    depth, S = 4, 16
    V = (np.random.default_rng(1000 * depth + 50).random((S, S, S)) < 0.5).astype(np.uint8)
    volume = volume_of(V)
    before = volume.editScratchBytes()
    volume.surfaceCount()
    assert volume.editScratchBytes() == before + offsets_bytes(depth) == before + 64
    check_volume(volume, V, "random 16")
    volume.close()


def test_depth_8_sparse_random_field(built):
    """256^3 at density 0.02: about two million faces in all 2048 slots.  Counts, the total by capacity 0 and every record,
    closed and open (the open list is the closed one without the faces on the volume's own walls); windows of records and
    triangles that begin at the first face of workgroup 1024, the first slot of the scan's second step, and just before"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 8, 256
    V = (np.random.default_rng(1000 * depth + 2).random((S, S, S)) < 0.02).astype(np.uint8)
    closed = F.faces(V, True)
    T = closed.shape[0]
    c = closed.astype(np.int64)
    axis, side = c[:, 3] >> 1, c[:, 3] & 1
    on_wall = c[np.arange(T), axis] == np.where(side == 1, S - 1, 0)
    per_word = F.word_direction_counts(closed, S)
    groups = per_word.shape[0] // 256
    assert groups == 2048 and scan_steps(groups) == 2 and T > 1900000 and (per_word.reshape(groups, -1).sum(axis=1) > 0).all()
    volume = volume_of(V)
    before = volume.editScratchBytes()
    volume.surfaceCount()
    assert volume.editScratchBytes() == before + offsets_bytes(depth)
    L = vrc.capi.load()
    for is_closed, want in ((True, closed), (False, closed[~on_wall])):
        counts = volume.surfaceCount(is_closed)
        assert np.array_equal(counts, F.direction_counts(want)), (is_closed, counts)
        total = C.c_uint64()
        assert L.vrc_volume_extract_surface(volume._h, int(is_closed), 0, 0, 0, None, C.byref(total), 0, None) == 0
        assert total.value == want.shape[0]
        got = volume.surfaceFaces(is_closed)
        assert got.shape == want.shape and np.array_equal(got, want), is_closed
    assert on_wall.sum() > 0
    edge = int(per_word.reshape(-1)[:6 * 256 * SCAN_GROUP].sum())       # the first face of workgroup 1024
    assert 0 < edge < T - 1000
    for first in (edge, edge - 1):
        want = closed[first:first + 300]
        assert np.array_equal(volume.surfaceFaces(True, first, 300), want), first
        assert np.array_equal(volume.surfaceTriangles(True, first, 300), F.triangles(want)), first
        for fmt, per, rows, expect in ((vrc.capi.VRC_SURFACE_FACES, 4, 1, want), (vrc.capi.VRC_SURFACE_TRIANGLES, 18, 2, F.triangles(want))):
            dev = torch.full((300 + 4, per), SENTINEL, dtype=torch.int32, device="cuda")
            dev_total = torch.zeros(1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            volume.extractSurfaceDevice(fmt, first, 300, dev.data_ptr(), dev_total.data_ptr())
            torch.cuda.synchronize()
            got = dev.cpu().numpy()
            assert int(dev_total.item()) == T
            assert np.array_equal(got[:300].reshape(-1, per // rows), expect.astype(np.int64).astype(np.int32)), (fmt, first)
            assert np.all(got[300:] == SENTINEL), (fmt, first)
    volume.close()


def test_depth_9_boxes(built):
    """512^3 through boxes: three groups of small boxes, at the origin corner, around the middle and at the far corner, each
    modelled in a 32^3 field with a margin to the field's sides that do not lie on the volume's walls, translated and
    ordered with the model's key at S = 512; then the full volume"""
    import cpuvoxelraycaster_amd as vrc
    depth, S, m = 9, 512, 32
    near = [[0, 0, 0, 3, 2, 5], [0, 6, 0, 1, 9, 1], [7, 0, 9, 12, 4, 11]]
    middle = [[5, 5, 5, 9, 17, 6], [11, 3, 8, 12, 4, 27], [20, 20, 2, 27, 22, 9]]
    far = [[m - 3, m - 2, m - 5, m, m, m], [m - 1, m - 9, m - 1, m, m - 6, m], [m - 12, m - 4, m - 11, m - 7, m, m - 9]]
    groups = ((near, 0), (middle, S // 2 - 17), (far, S - m))
    volume = vrc.VoxelVolume(depth)
    volume.fillBoxes([[c + off for c in box] for boxes, off in groups for box in boxes])
    before = volume.editScratchBytes()
    volume.surfaceCount()
    assert volume.editScratchBytes() == before + offsets_bytes(depth) == before + 8 * (16384 + 7)
    for closed in (True, False):
        parts = []
        for boxes, off in groups:
            V = np.zeros((m, m, m), np.uint8)
            for x0, y0, z0, x1, y1, z1 in boxes:
                V[x0:x1, y0:y1, z0:z1] = 1
            if boxes is middle:
                assert not V[0].any() and not V[m - 1].any() and not V[:, 0].any() and not V[:, m - 1].any() and not V[:, :, 0].any() and not V[:, :, m - 1].any()
            else:
                assert not V[m // 2].any() and not V[:, m // 2].any() and not V[:, :, m // 2].any()
            f = F.faces(V, True if boxes is middle else closed).astype(np.int64)
            f[:, :3] += off
            parts.append(f)
        want = F.ordered(np.concatenate(parts), S)
        assert np.array_equal(volume.surfaceCount(closed), F.direction_counts(want)), closed
        got = volume.surfaceFaces(closed)
        assert np.array_equal(got, want), closed
        assert np.array_equal(volume.surfaceTriangles(closed), F.triangles(want)), closed
        assert got[:, :3].max() == S - 1 and got[:, :3].min() == 0
    k = int(np.argmax(want[:, 0] >= S - m))
    assert 0 < k < want.shape[0] - 7 and np.array_equal(volume.surfaceFaces(False, k, 7), want[k:k + 7])
    volume.fillBoxes([[0, 0, 0, S, S, S]])
    assert np.array_equal(volume.surfaceCount(True), np.full(6, S * S, np.uint64)) and volume.surfaceCount(False).sum() == 0
    wall = volume.surfaceFaces(True, 0, 1000)
    assert wall.shape == (1000, 4) and np.array_equal(F.ordered(wall, S), wall)
    volume.close()
