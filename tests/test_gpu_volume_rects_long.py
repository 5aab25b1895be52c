"""Merged-rectangle extraction on the GPU where a run of faces spans several words of a row (csrc/vrc_rects.hip: run_end
beyond the next word, holds_run in a middle word and at the bit beside a word-aligned end, both carries of rect_starts), and
at the depths tests/test_gpu_volume_rects.py leaves out: 4 (the first at which a workgroup lies inside one direction, the
last that gathers bit by bit), 8 and 9 (8 and 16 words a row; 12 288 and 98 304 slots, 12 and 96 steps of the scan).  The
scenes are tests/rect_cases.py's, which tests/test_volume_rect_cases_host.py holds to these paths without a GPU and under
which emulated wrong kernels change the records.  Every comparison is exact and in the canonical order: against
rect_model.rects up to 128^3, against the plane-by-plane sparse model (held equal to it there) at 256^3 and 512^3."""
import ctypes as C
import functools

import numpy as np
import pytest

import rect_cases as K
import rect_model as R
from test_gpu_volume_rects import SENTINEL, block_bytes, check_volume
from volume_support import volume_of

pytestmark = pytest.mark.gpu


def filled(scene):
    """the scene on the device, made the way the scene was: boxes, or cells then holes then specks"""
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(scene.depth)
    if scene.boxes is not None:
        volume.fillBoxes(scene.boxes)
    else:
        volume.fillBoxes(scene.cells)
        volume.setVoxels(scene.holes, False)
        volume.setVoxels(scene.specks)
    return volume


@functools.lru_cache(maxsize=None)
def wanted(scene, closed):
    """the model's records: dense up to 128^3, plane by plane above"""
    r = R.rects(scene.dense(), closed) if scene.depth <= 7 else K.sparse_rects(scene.planes(), closed)
    r.setflags(write=False)
    return r


def check_scene(scene, volume=None):
    volume = volume or filled(scene)
    before = volume.editScratchBytes()
    volume.rectCount()
    assert volume.editScratchBytes() == before + block_bytes(scene.depth)
    check_volume(volume, None, scene.name, lambda closed: wanted(scene, closed))
    if scene.axis is not None:
        assert np.array_equal(K.sheet_records(volume.surfaceRects(False), scene.axis), scene.expected), scene.name
    return volume


# ---- 16^3 -----------------------------------------------------------------------------------------------------------------

def test_depth_4(built):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 4, 16
    V = (np.random.default_rng(2000 * depth + 50).random((S, S, S)) < 0.5).astype(np.uint8)
    volume = volume_of(V)
    before = volume.editScratchBytes()
    volume.rectCount()
    assert volume.editScratchBytes() == before + block_bytes(depth) == before + 8 * (6 + 7) + 8 * 256
    check_volume(volume, V, "random")
    volume.close()
    board = (np.indices((S, S, S)).sum(axis=0) & 1).astype(np.uint8)
    corners = np.zeros((S, S, S), np.uint8)
    corners[::S - 1, ::S - 1, ::S - 1] = 1
    for what, V in (("empty", np.zeros((S, S, S), np.uint8)), ("full", np.ones((S, S, S), np.uint8)), ("checkerboard", board), ("corners", corners),
                    ("constructed", K.small_constructed(S))):
        volume = volume_of(V)
        check_volume(volume, V, what)
        if what == "full":
            u = vrc.VoxelVolume.unpackRects(volume.surfaceRects())
            assert u.shape == (6, 6) and np.all(u[:, 4:] == S) and volume.rectCount(False).sum() == 0
        if what == "corners":
            assert volume.rectCount(True).sum() == 48 and volume.rectCount(False).sum() == 24
        if what == "constructed":
            up = vrc.VoxelVolume.unpackRects(volume.surfaceRects(False))
            assert up[(up[:, 3] == 3) & (up[:, 1] == 7)].tolist() == K.SMALL_UP
        volume.close()
    for axis in range(3):
        for side in (0, 1):
            scene = K.slab(depth, axis, side)
            volume = filled(scene)
            check_volume(volume, scene.dense(), scene.name)
            assert volume.rectCount(True).sum() == 6 and volume.rectCount(False).sum() == 1
            volume.close()


# ---- 128^3: four words a row ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pair_table_128(built, axis):
    check_scene(K.pair_table(7, axis)).close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_stacks_128(built, axis):
    check_scene(K.stacks(7, axis)).close()


@pytest.mark.parametrize("run_axis", [2, 1])
def test_blocky_128(built, run_axis):
    scene = K.blocky(7, run_axis)
    volume = check_scene(scene)
    assert np.array_equal(volume.download(), scene.dense())
    volume.close()


def test_windows_at_the_second_step_of_the_scan(built):
    """windows that begin at the first record of workgroup 1024 -- the first slot of the scan's second step -- and at the
    record before it, in host and device memory, a sentinel behind what is written; triangles once through the narrow
    stores"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    scene = K.blocky(7, 2)
    want = wanted(scene, True)
    want_tris = R.triangles(want)
    T = want.shape[0]
    group = K.lane_of(want, scene.S) // K.GROUP
    edge = int(np.searchsorted(group, K.SCAN_GROUP))
    assert 0 < edge < T - 40 and group[edge - 1] < K.SCAN_GROUP <= group[edge]
    volume = filled(scene)
    L = vrc.capi.load()
    for fmt, per, rows, expect in ((vrc.capi.VRC_SURFACE_FACES, 4, 1, want), (vrc.capi.VRC_SURFACE_TRIANGLES, 18, 2, want_tris)):
        dtype = np.uint32 if fmt == vrc.capi.VRC_SURFACE_FACES else np.int32
        for first in (edge, edge - 1):
            for cap in (1, 2, 37, T):
                n = min(cap, T - first)
                buf = np.full((n + 4, per), SENTINEL, dtype)
                total = C.c_uint64()
                vrc.capi.check(L.vrc_extract_rects(volume._h, 1, fmt, first, cap, vrc.capi.ptr(buf), C.byref(total), 0, None))
                assert total.value == T
                assert np.array_equal(buf[:n].reshape(-1, per // rows), expect[rows * first:rows * (first + n)]), (fmt, first, cap)
                assert np.all(buf[n:] == SENTINEL), (fmt, first, cap)
                dev = torch.full((n + 4, per), SENTINEL, dtype=torch.int32, device="cuda")
                dev_total = torch.zeros(1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                volume.extractRectsDevice(fmt, first, cap, dev.data_ptr(), dev_total.data_ptr())
                torch.cuda.synchronize()
                got = dev.cpu().numpy().view(dtype)
                assert int(dev_total.item()) == T
                assert np.array_equal(got[:n].reshape(-1, per // rows), expect[rows * first:rows * (first + n)]), (fmt, first, cap, "device")
                assert np.all(got[n:] == SENTINEL), (fmt, first, cap, "device")
    dev = torch.full((1 + 18 * 10 + 3,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    volume.extractRectsDevice(vrc.capi.VRC_SURFACE_TRIANGLES, edge - 1, 10, dev.data_ptr() + 4, None)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(got[1:181].reshape(-1, 9), want_tris[2 * (edge - 1):2 * (edge - 1) + 20]) and np.all(got[181:] == SENTINEL) and got[0] == SENTINEL
    volume.close()


# ---- 256^3: eight words a row, twelve steps of the scan -----------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pair_table_and_stacks_256(built, axis):
    check_scene(K.pair_table(8, axis)).close()
    check_scene(K.stacks(8, axis)).close()


def test_blocky_256(built):
    scene = K.blocky(8, 2)
    assert wanted(scene, True).shape[0] < 1 << 20
    check_scene(scene).close()


# ---- 512^3: sixteen words a row, ninety-six steps ---------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pair_table_512(built, axis):
    check_scene(K.pair_table(9, axis)).close()


def test_stacks_full_volume_and_slabs_512(built):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 9, 512
    for axis in range(3):
        check_scene(K.stacks(depth, axis)).close()
    full = K.full_volume(depth)
    volume = check_scene(full)
    got = volume.surfaceRects(True)
    assert np.array_equal(got, full.expected) and np.all(vrc.VoxelVolume.unpackRects(got)[:, 4:] == S) and volume.rectCount(False).sum() == 0
    volume.close()
    for axis in range(3):
        for side in (0, 1):
            volume = check_scene(K.slab(depth, axis, side))
            assert volume.rectCount(True).sum() == 6 and volume.rectCount(False).sum() == 1
            volume.close()
