"""vrc_morph_apply where k_morph_apply (csrc/vrc_morph.hip) can first go wrong without test_gpu_volume_morph.py noticing: on
results that are not a constant, and in tiles that have neighbours on every side.  The cases are tests/morph_cases.py's,
held to their conditions without a GPU in tests/test_morph_cases_host.py: sources tuned to the element, so that the model's
result is half solid and every offset decides voxels; 128^3 and 256^3, the first sizes with interior tiles and z blocks, where
the volume's brick rows (64, 128) and words per row (16, 32) are no constant of the kernel; 512^3 and 1024^3 from lists of
coordinates, for the 32-bit word index and the high tile numbers; the list at its cap of 2^20 offsets; and two calls into
one destination from two streams, which share the destination's block for the prepared element.  Every expected value comes
from morph_model.py or from a list of coordinates on the host, never from another GPU result; every comparison is exact.

Measured on the MI355X, per test: the unsaturated elements 0.01 .. 0.05 s at 32^3 and 64^3, 0.03 .. 0.15 s at 128^3 and
0.22 .. 0.41 s at 256^3 (slab33 the slowest at both); the translations at 128^3 0.05 s for each `outside`; the lists at 512^3
and 1024^3 0.01 .. 0.04 s an element (ball3 the slowest); the list at its cap 0.45 s; the two streams 0.03 s an order.  The 97
tests take 8.9 s together after the library's set-up, next to 0.84 s for the slowest test of test_gpu_volume_morph.py in the
same run (test_one_voxel_by_every_small_offset[8-0]) and 7.9 s for that file; none skips."""
import numpy as np
import pytest

import cells_model
import morph_cases as cases
import morph_model as model
from volume_support import Stream

pytestmark = pytest.mark.gpu

DILATE, ERODE, SOLID, EMPTY = model.DILATE, model.ERODE, model.SOLID, model.EMPTY
REPLACE, OR, ANDNOT = model.REPLACE, model.OR, model.ANDNOT
_GARBAGE = {}


def depth_of(S):
    return S.bit_length() - 1


def garbage(S):
    """fillRandom(5, 0.5)'s set, dense [x, y, z].  Shared: do not write to it."""
    if S not in _GARBAGE:
        _GARBAGE[S] = cells_model.random_set(5, cells_model.threshold_of(0.5), S)
        _GARBAGE[S].setflags(write=False)
    return _GARBAGE[S]


def upload(vol):
    """a volume that holds `vol`, sent as the list of the rarer kind of voxel"""
    import cpuvoxelraycaster_amd as vrc
    S = vol.shape[0]
    volume = vrc.VoxelVolume(depth_of(S))
    if 2 * int(vol.sum()) > S ** 3:
        volume.fillBoxes([[0, 0, 0, S, S, S]])
        volume.setVoxels(np.argwhere(vol == 0), False)
    elif vol.any():
        volume.setVoxels(np.argwhere(vol))
    return volume


def same(got, want, what):
    """bit for bit, or the count, the first differing voxels and the (x tile, y tile, z block) they lie in"""
    if got.shape == want.shape and np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    blocks = np.unique(cases.tile_of(bad), axis=0)
    raise AssertionError("%s: %d voxels differ in %d workgroups' blocks, the first at %s in (tile x, tile y, z block) %s; got there %s" % (
        what, len(bad), len(blocks), bad[:4].tolist(), cases.tile_of(bad[:4]).tolist(), got[tuple(bad[:4].T)].tolist()))


def before_call(dst, S, pattern):
    """what the call finds in dst: nothing, everything, or fillRandom's set; returns it dense"""
    if pattern == 2:
        dst.fillRandom(5, 0.5, None, REPLACE)
        return garbage(S)
    dst.fillBoxes([[0, 0, 0, S, S, S]], bool(pattern))
    return np.full((S, S, S), pattern, np.uint8)


# ---- 1. unsaturated elements ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_unsaturated_elements(built, name, S):
    """every form of forms_of(name, S) on the source tuned to the element and the form; the three ops and the three
    destination patterns cycle as Bench.check's do.  The piece goes through device memory: its voxel list about a pivot"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    e = cases.elements()[name]
    vols = {sparse: cases.tuned_source(name, S, sparse) for sparse in (True, False)}
    srcs = {sparse: upload(vol) for sparse, vol in vols.items()}
    dst = vrc.VoxelVolume(depth_of(S))
    if name == "piece":
        piece = upload(cases.piece_shape())
        listed = torch.full((len(e) + 2, 3), 0x7B7B7B7B, dtype=torch.int32).cuda()      # a canary row on either side of the list
        torch.cuda.synchronize()
    for i, (what, of, outside) in enumerate(cases.forms_of(name, S)):
        calls = cases.NAMES.index(name) + i
        op, pattern = calls % 3, (calls // 3) % 3
        sparse = cases.ored_is_sparse_solid(what, of)
        before = before_call(dst, S, pattern)
        if name == "piece":
            with Stream() as stream:
                piece.extractVoxelsDevice(capi.VRC_VOXELS_ALL, capi.VRC_VOXELS_XYZ, 0, len(e), listed.data_ptr() + 12, None, stream=stream)
                assert srcs[sparse].morphDevice(dst, what, len(e), listed.data_ptr() + 12, cases.PIECE_PIVOT, of == EMPTY, bool(outside), op, stream=stream) is dst
                got = dst.download()
        else:
            assert srcs[sparse].morph(what, e, dst, of == EMPTY, bool(outside), op) is dst
            got = dst.download()
        want = model.apply_op(before, model.morph_words(vols[sparse], what, e, of, outside), op)
        same(got, want, (name, S, what, of, outside, op, pattern))
    if name == "piece":
        rows = listed.cpu().numpy()
        assert (rows[0] == 0x7B7B7B7B).all() and (rows[-1] == 0x7B7B7B7B).all()
        assert sorted((rows[1:-1] - np.array(cases.PIECE_PIVOT, np.int32)).tolist()) == sorted(e.tolist())
        piece.close()
    for sparse, src in srcs.items():
        same(src.download(), vols[sparse], (name, S, "the source is only read"))
        src.close()
    dst.close()


# ---- 2. translations where tiles are interior ---------------------------------------------------------------------------------

def interior_offsets():
    from test_gpu_volume_morph import single_offsets
    corners = single_offsets()[1]
    alone = [tuple(v if a == axis else 0 for a in range(3)) for axis in range(3) for v in (-16, -15, -1, 1, 15, 16)]
    assert len(corners) == 27 and len(set(corners + alone)) == 45
    return corners + alone


@pytest.mark.parametrize("outside", [0, 1])
def test_single_offsets_are_translations_at_128(built, outside):
    import cpuvoxelraycaster_amd as vrc
    S = 128
    vol = cells_model.random_set(128, cells_model.threshold_of(0.5), S)
    src, dst = upload(vol), vrc.VoxelVolume(depth_of(S))
    padded = np.pad(vol, 16, constant_values=outside)
    for e in interior_offsets():
        dst.fillBoxes([[0, 0, 0, S, S, S]])
        src.morph(DILATE, [e], dst, outside=bool(outside))
        want = padded[16 - e[0]:16 - e[0] + S, 16 - e[1]:16 - e[1] + S, 16 - e[2]:16 - e[2] + S]         # K(p) = A(p - e)
        same(dst.download(), want, (S, outside, e))
    src.close()
    dst.close()


# ---- 3. 512^3 and 1024^3 from lists ---------------------------------------------------------------------------------------------

def check_whole_volume(volume, want, what):
    """the volume holds exactly the voxels `want` (in list order, without repetitions): the count, then the whole list"""
    assert volume.solidCount() == len(want), (what, volume.solidCount(), len(want))
    got = volume.voxels().astype(np.int64)
    if not (got.shape == want.shape and np.array_equal(got, want)):
        have, need = {tuple(v) for v in got.tolist()}, {tuple(v) for v in want.tolist()}
        extra, missing = sorted(have - need)[:4], sorted(need - have)[:4]
        raise AssertionError("%s: extra %s in blocks %s, missing %s in blocks %s" % (what, extra, cases.tile_of(extra).tolist() if extra else [],
                                                                                  missing, cases.tile_of(missing).tolist() if missing else []))


@pytest.fixture(scope="module", params=[512, 1024])
def large(request, built):
    """(S, the volume of sparse_points(S), the full volume without them, a destination, a third volume): one of each per size,
    made once for the module.  The erosion wants a source of its own, the complement of the dilation's, so there are two
    sources a size where a single 1024^3 source per module was asked for: four volumes of 128 MiB, 512 MiB, alive together
    at 1024^3, after those of 512^3 are closed."""
    import cpuvoxelraycaster_amd as vrc
    S = request.param
    p = cases.sparse_points(S).astype(np.uint32)
    made = [vrc.VoxelVolume(depth_of(S)) for _ in range(4)]
    made[0].setVoxels(p)
    made[1].fillBoxes([[0, 0, 0, S, S, S]])
    made[1].setVoxels(p, False)
    assert made[0].solidCount() == len(p) and made[1].solidCount() == S ** 3 - len(p)
    yield (S,) + tuple(made)
    for v in made:
        v.close()


@pytest.mark.parametrize("name", cases.LARGE_ELEMENTS)
def test_dilate_and_erode_from_lists(large, name):
    """DILATE under REPLACE into a destination that is solid throughout: every word has to be written for the result to be the
    sparse list.  ERODE (outside = 1) of the full volume with holes: the count, and the complete list of the complement, taken
    with the zero offset `of_empty` into a third volume"""
    S, solid, holed, dst, third = large
    e, p = cases.elements()[name], cases.sparse_points(S)
    dst.fillBoxes([[0, 0, 0, S, S, S]])
    assert dst.solidCount() == S ** 3
    assert solid.morph(DILATE, e, dst) is dst
    check_whole_volume(dst, cases.dilated(p, e, S), (S, name, "dilate"))
    want = cases.erosion_holes(p, e, S)
    holed.morph(ERODE, e, dst, outside=True)
    assert dst.solidCount() == S ** 3 - len(want), (S, name, dst.solidCount(), S ** 3 - len(want))
    third.fillBoxes([[0, 0, 0, S, S, S]])
    dst.morph(DILATE, [(0, 0, 0)], third, of_empty=True)
    check_whole_volume(third, want, (S, name, "the complement of the erosion"))
    assert solid.solidCount() == len(p) and holed.solidCount() == S ** 3 - len(p)


# ---- 4. the list at its cap -------------------------------------------------------------------------------------------------------

def test_the_list_at_its_cap(built):
    """2^20 offsets, 100 distinct: from host memory and from device memory, both the model of the 100"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 32
    e, rows = cases.capped_list()
    t_rows = torch.from_numpy(rows.copy()).cuda()
    torch.cuda.synchronize()
    dst = vrc.VoxelVolume(depth_of(S))
    for what, of, outside in ((DILATE, SOLID, 0), (ERODE, SOLID, 1)):
        vol = cases.source_for(len(e), 32100, S, cases.ored_is_sparse_solid(what, of))
        src = upload(vol)
        scratch = (src.editScratchBytes(), dst.editScratchBytes())
        want = model.morph(vol, what, e, of, outside)
        assert 0.03 * S ** 3 < want.sum() < 0.97 * S ** 3
        before_call(dst, S, 2)
        src.morph(what, rows, dst, outside=bool(outside))
        same(dst.download(), want, ("host memory", what))
        before_call(dst, S, 2)
        with Stream() as stream:
            src.morphDevice(dst, what, len(rows), t_rows.data_ptr(), outside=bool(outside), stream=stream)
            got = dst.download()
        same(got, want, ("device memory", what))
        assert (src.editScratchBytes(), dst.editScratchBytes()) == scratch
        src.close()
    assert np.array_equal(t_rows.cpu().numpy(), rows)
    dst.close()


# ---- 5. one destination, two streams ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swapped", [False, True])
def test_two_streams_into_one_destination(built, swapped):
    """REPLACE on one stream, then OR with another element on a second: the second call prepares its element in the block the
    first one's kernel reads, and only the library's ordering of dst's edits keeps them apart"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 128
    first, second = cases.elements()["ball5"], cases.elements()["random48"]
    if swapped:
        first, second = second, first
    vol = cases.source_for(len(first) + len(second), 128200, S)
    k1, k2 = model.morph_words(vol, DILATE, first), model.morph_words(vol, DILATE, second)
    want = model.apply_op(model.apply_op(garbage(S), k1, REPLACE), k2, OR)
    assert not np.array_equal(want, k1) and not np.array_equal(want, k2) and 0.2 < want.mean() < 0.8
    src, dst = upload(vol), vrc.VoxelVolume(depth_of(S))
    before_call(dst, S, 2)
    t1, t2 = torch.from_numpy(first.copy()).cuda(), torch.from_numpy(second.copy()).cuda()
    torch.cuda.synchronize()
    with Stream() as a, Stream() as b:
        src.morphDevice(dst, DILATE, len(first), t1.data_ptr(), stream=a)
        src.morphDevice(dst, DILATE, len(second), t2.data_ptr(), op=OR, stream=b)
        got = dst.download()
    same(got, want, ("two streams", swapped))
    src.close()
    dst.close()
