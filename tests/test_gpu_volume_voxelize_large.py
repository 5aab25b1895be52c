"""vrc_volume_xor_mesh where the column scan spans a wave and the mark loop strides: the scan at 2, 16, 32 and 64 lanes a
brick column and at two words a lane (depths 4, 7, 8, 9, 10), the mark loop in its second and later steps under split = 1
(depth 5), 1 < split < useful (depth 7) and the cap of 1024 workgroups a triangle (depth 10), and stampMesh through a 256^3
clipboard.  The cases, their expected flips and the geometry they reach are tests/voxelize_cases.py's, held to their
conditions -- and to the numpy model -- in tests/test_volume_voxelize_cases_host.py.  Every comparison is exact.  How a
result is read back: the records of diff() against a clone made before the call, which name every occupancy word that
changed and the bits that did, against the expected flips word for word -- so every other word is bit-identical --; then,
up to 256^3, the whole downloaded volume against the dense expectation, and at 512^3 and 1024^3 every touched column by
getVoxels (the sheets) or every run by countBoxes (the slabs), with solidCount against the expectation's total.  After
each call the same triangles again must give the volume back: diff() has no record.

Measured on the MI355X: the ten tests of this file take 3.2 s together, the library's set-up included, the slowest (1024^3)
0.34 s; none skips."""

import numpy as np
import pytest

import voxelize_cases as cases
import voxelize_model as M

pytestmark = pytest.mark.gpu


def records(before, volume):
    delta = before.diff(volume)
    rec = delta.records()
    delta.close()
    return rec["word"].astype(np.int64), rec["bits"]


def column_voxels(flips, S):
    """every voxel of every column the flips touch, as (n, 3) coordinates, and the expected flip of each"""
    cols = np.unique(flips[:, :2], axis=0)
    xyz = np.concatenate([np.repeat(cols, S, axis=0), np.tile(np.arange(S), len(cols))[:, None]], axis=1)
    key = flips[:, 0] * S + flips[:, 1]
    index = np.searchsorted(np.unique(key), key)
    marks = np.zeros((len(cols), S + 1), np.uint8)
    marks[index, flips[:, 2]] = 1
    want = np.bitwise_xor.accumulate(marks[:, :0:-1], axis=1)[:, ::-1]
    return xyz, want.reshape(-1)


def xor_and_check(volume, depth, tris, flips, boxes=None, by_runs=False):
    """one xorMesh into the volume (empty, or holding the boxes), checked as the module's docstring says, and undone"""
    S = 1 << depth
    boxes = np.zeros((0, 6), np.uint32) if boxes is None else boxes
    before = volume.clone()
    volume.xorMesh(tris)
    words, bits = records(before, volume)
    want_words, want_bits = cases.flip_words(depth, flips)
    assert len(words) == len(want_words), (depth, len(words), len(want_words))
    assert np.array_equal(words, want_words) and np.array_equal(bits, want_bits), (depth, np.flatnonzero((words != want_words) | (bits != want_bits))[:5])
    runs = M.runs_of_flips(flips)
    total = cases.boxes_volume(boxes) + M.count_of_flips(flips) - 2 * cases.solid_in_boxes(boxes, runs) if len(boxes) else M.count_of_flips(flips)
    assert volume.solidCount() == total, (depth, volume.solidCount(), total)
    if depth <= 8:
        want = M.dense_of_flips(S, flips, cases.dense_boxes(S, boxes))
        got = volume.download()
        assert np.array_equal(got, want), (depth, np.argwhere(got != want)[:5].tolist())
    elif by_runs:
        assert not len(boxes)
        counts = volume.countBoxes(np.concatenate([runs[:, :3], runs[:, :2] + 1, runs[:, 3:]], axis=1))
        assert np.array_equal(counts.astype(np.int64), runs[:, 3] - runs[:, 2])
    else:
        xyz, flipped = column_voxels(flips, S)
        was = np.zeros(len(xyz), np.uint8)
        for x0, y0, z0, x1, y1, z1 in boxes.astype(np.int64).tolist():
            was |= ((xyz >= (x0, y0, z0)) & (xyz < (x1, y1, z1))).all(axis=1)
        got = volume.getVoxels(xyz)
        assert np.array_equal(got, was ^ flipped), (depth, xyz[np.flatnonzero(got != (was ^ flipped))[:5]].tolist())
    volume.xorMesh(tris)                                                    # the involution; the mark field went back to zero
    delta = before.diff(volume)
    assert delta.count == 0, (depth, delta.count)
    delta.close()
    assert volume.solidCount() == cases.boxes_volume(boxes)
    before.close()


def scan_cases_at(depth):
    import cpuvoxelraycaster_amd as vrc
    case = cases.scan_case(depth)
    volume = vrc.VoxelVolume(depth)
    xor_and_check(volume, depth, case.tris, case.flips)
    boxes = cases.before_boxes(depth)
    volume.fillBoxes(boxes)
    xor_and_check(volume, depth, case.tris, case.flips, boxes)
    return volume


# ---- the column scan --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [4, 7, 8])
def test_scan_over_2_16_and_32_lanes(built, depth):
    """word borders, two crossings a column, neighbours in a wave, cancelled marks and a random layer of sheets, into an empty
    volume and into one that holds solid voxels in the touched columns and elsewhere"""
    scan_cases_at(depth).close()


def test_scan_over_a_whole_wave_at_512(built):
    """64 lanes a column: the guard `pos + d < lanes` is all that keeps a lane from reading beyond the wave"""
    scan_cases_at(9).close()


# ---- the mark loop ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth, n", [(5, None), (7, 128), (7, 150)])
def test_mark_loop_strides(built, depth, n):
    """slab pairs over the whole volume: four steps a triangle on one workgroup among 4112 triangles at 32^3; two full steps
    (n = 128) and three with a partial last one (n = 150) at 128^3"""
    import cpuvoxelraycaster_amd as vrc
    case = cases.stride_case(depth, n)
    volume = vrc.VoxelVolume(depth)
    xor_and_check(volume, depth, case.tris, case.flips)
    volume.close()


def test_mark_loop_strides_at_512(built):
    """eight triangles, 512 workgroups each: 262144 columns on 131072 lanes, two steps"""
    import cpuvoxelraycaster_amd as vrc
    case = cases.stride_case(9)
    volume = vrc.VoxelVolume(9)
    xor_and_check(volume, 9, case.tris, case.flips, by_runs=True)
    volume.close()


def test_depth_10_once(built):
    """1024^3, once: a slab pair over all 2^20 columns with corners at +-2^17 units (four triangles, the cap of 1024
    workgroups each, four steps of 262144 lanes; the largest products the rule meets here, |N| + D = 2^52.1), then in the
    same volume the scan cases at two words a lane -- sheets in columns (0, 0) and (1023, 1023) among them -- and those
    again into a volume that holds solid voxels.  No S^3 array on the host"""
    import cpuvoxelraycaster_amd as vrc
    depth = 10
    slab, sheets = cases.stride_case(depth), cases.scan_case(depth)
    cols = {(int(x), int(y)) for x, y, k in sheets.flips}
    assert (0, 0) in cols and (1023, 1023) in cols
    volume = vrc.VoxelVolume(depth)
    xor_and_check(volume, depth, slab.tris, slab.flips, by_runs=True)
    xor_and_check(volume, depth, sheets.tris, sheets.flips)
    boxes = cases.before_boxes(depth)
    volume.fillBoxes(boxes)
    xor_and_check(volume, depth, sheets.tris, sheets.flips, boxes)
    assert volume.editScratchBytes() >= 1 << 27                                # the mark field: a byte per brick
    volume.close()


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_stamp_an_icosphere_through_a_256_clipboard(built, heights):
    """stampMesh: an icosphere 150 voxels across through a 256^3 clipboard (32 lanes a column) into the 256^3 terrain with OR
    at an odd offset, against terrain | the model's ball"""
    import cpuvoxelraycaster_amd as vrc
    from volume_support import terrain_volume
    depth, S = cases.STAMP["depth"], 256
    terrain = terrain_volume(heights, depth)
    volume = vrc.VoxelVolume(depth)
    volume.fillBoxes(column_boxes(terrain))
    assert np.array_equal(volume.download(), terrain)
    verts, faces = vrc.icosphere(cases.STAMP["subdivisions"])
    lo, size = volume.stampMesh(verts, faces, vrc.capi.VRC_COPY_OR, cases.STAMP["radius"], cases.STAMP["centre"])
    assert 128 < max(size) <= 256 and any(v % 2 for v in lo)
    ball = M.dense_of_flips(S, cases.stamp_flips(verts, faces))
    assert (ball & terrain).any() and (ball & (1 - terrain)).sum() > 500000
    got = volume.download()
    assert np.array_equal(got, terrain | ball), np.argwhere(got != (terrain | ball))[:5].tolist()
    volume.close()


def column_boxes(terrain):
    """the terrain (solid for y in a range per (x, z)) as one box per column"""
    S = terrain.shape[0]
    x, z = [g.reshape(-1) for g in np.meshgrid(np.arange(S), np.arange(S), indexing="ij")]
    y0 = terrain.argmax(axis=1).reshape(-1)
    y1 = y0 + terrain.sum(axis=1, dtype=np.int64).reshape(-1)
    keep = y1 > y0
    return np.stack([x, y0, z, x + 1, y1, z + 1], axis=1)[keep].astype(np.uint32)
