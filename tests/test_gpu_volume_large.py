"""The voxel-volume kernels where a loop takes its second step: the labelling at 256^3, whose slot scan (vrc_group.h:
scan_slots) carries the roots of the first 1024 workgroups into the ids of the second 1024; a serpentine through all 256
workgroups of 128^3; copyRegion and the affine stamp at 512^3, where box_launch_groups caps the launch and the first 65536
lanes take a second word; and the box and sphere lists under split_for.  The cases, the expected results and the geometry
they reach are tests/large_volume_cases.py's, held to their conditions in tests/test_volume_large_cases_host.py.  The
expected values come from numpy (components_model, stamp_model, slices), never from another GPU result, and every
comparison is exact."""

import numpy as np
import pytest

import components_model
import large_volume_cases as cases
import rigid_model
import stamp_model
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu
NONE = cases.NONE


def apply(volume, edits):
    for kind, items, solid in edits:
        {"boxes": volume.fillBoxes, "voxels": volume.setVoxels, "spheres": volume.fillSpheres}[kind](items, bool(solid))
    return volume


def same(got, want, what):
    """np.array_equal, with the first few differing coordinates in the message"""
    if not np.array_equal(got, want):
        where = np.argwhere(got != want)
        raise AssertionError("%s: %d voxels differ, the first at %s" % (what, len(where), where[:5].tolist()))


# ---- 1. the labelling at 256^3 ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene(built):
    case = cases.labelling_case()
    medium = volume_of(case.vol)
    content = apply(type(medium)(8), cases.content_edits(256))
    yield case, medium, content, cases.dense_of(cases.content_edits(256), 256)
    medium.close()
    content.close()


def check_labels(labels, case, connectivity, what):
    """count, every record, at() on the sample and bytes()"""
    ids, rec = case.ids[connectivity], case.rec[connectivity]
    assert labels.count == len(rec), (what, labels.count, len(rec))
    got = labels.components()
    for field in ("first", "lo", "hi", "reserved", "voxels"):
        bad = np.flatnonzero((got[field] != rec[field]).reshape(len(rec), -1).any(axis=1))
        assert not len(bad), (what, field, len(bad), bad[:5].tolist())
    xyz = cases.at_sample(case, connectivity)
    at = labels.at(xyz)
    want = ids[tuple(xyz.astype(np.int64).T)]
    bad = np.flatnonzero(at != want)
    assert not len(bad), (what, len(bad), xyz[bad[:5]].tolist(), at[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert labels.bytes() == 4 * 256 ** 3 + 48 * len(rec)


def check_select(labels, case, connectivity, content, content_vol):
    """a keep mask with pieces on both sides of the boundary: REPLACE into a fresh volume, OR and ANDNOT into the slabs"""
    keep = cases.keep_mask(case, connectivity)
    slots = cases.root_slots(case.rec[connectivity], 256)
    assert keep[slots < 1024].any() and keep[slots >= 1024].any() and not keep[slots < 1024].all() and not keep[slots >= 1024].all()
    K = components_model.select(case.ids[connectivity], keep)
    fresh = labels.select(keep)
    got = fresh.download()
    fresh.close()
    same(got, K, ("select REPLACE", connectivity))
    for op in (cases.OR, cases.ANDNOT):
        dst = content.clone()
        labels.select(keep, dst, op)
        got = dst.download()
        dst.close()
        want = cases.apply_op(content_vol, K, op)
        assert not np.array_equal(want, content_vol)
        same(got, want, ("select", op, connectivity))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_labelling_at_256_numbers_the_pieces_beyond_slot_1024(scene, connectivity):
    """2048 slots: the ids of every piece whose root lies at x >= 128 come out of the scan's second step"""
    case, medium, content, content_vol = scene
    labels = medium.labelComponents(connectivity)
    check_labels(labels, case, connectivity, connectivity)
    check_select(labels, case, connectivity, content, content_vol)
    labels.close()


def test_labelling_at_256_through_the_empty_voxels(scene):
    """the complement of the scene labelled through its empty voxels: the same pieces"""
    import cpuvoxelraycaster_amd as vrc
    case = scene[0]
    hollow = vrc.VoxelVolume(8)
    hollow.fillBoxes([[0, 0, 0, 256, 256, 256]])
    hollow.setVoxels(np.argwhere(case.vol), False)
    labels = hollow.labelComponents(6, True)
    hollow.close()
    check_labels(labels, case, 6, "through empty")
    labels.close()


def test_labelling_at_256_device_memory_forms_and_moments(scene):
    """at, components (a window that starts below the boundary's first id and runs past the end) and select in device memory
    on a created stream; then moments(), so that the rigid kernels read ids from beyond the carry"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    case, medium, content, content_vol = scene
    ids, rec = case.ids[6], case.rec[6]
    Cn = len(rec)
    labels = medium.labelComponents(6)
    assert labels.count == Cn
    xyz = cases.at_sample(case, 6)
    keep = cases.keep_mask(case, 6)
    first = int((cases.root_slots(rec, 256) < 1024).sum()) - 100
    t_xyz = torch.from_numpy(xyz.view(np.int32)).cuda()
    t_ids = torch.full((len(xyz),), 5, dtype=torch.int32).cuda()
    t_rec = torch.full((48 * (Cn - first + 2),), 0xAB, dtype=torch.uint8).cuda()
    t_keep = torch.from_numpy(keep).cuda()
    dst = content.clone()
    torch.cuda.synchronize()
    with Stream() as stream:
        labels.atDevice(len(xyz), t_xyz.data_ptr(), t_ids.data_ptr(), stream)
        labels.componentsDevice(first, Cn - first + 2, t_rec.data_ptr(), stream)
        labels.selectDevice(t_keep.data_ptr(), dst, cases.OR, stream)
        got = dst.download()                                  # ordered behind the device-memory select
    dst.close()
    assert np.array_equal(t_ids.cpu().numpy().view(np.uint32), ids[tuple(xyz.astype(np.int64).T)])
    raw = t_rec.cpu().numpy()
    assert raw[:48 * (Cn - first)].tobytes() == rec[first:].tobytes() and (raw[48 * (Cn - first):] == 0xAB).all()
    same(got, content_vol | components_model.select(ids, keep), "selectDevice OR")
    want = np.array([[n] + list(s1) + list(s2) for n, s1, s2 in rigid_model.moments_fast(ids, Cn)], np.uint64)
    m = labels.moments()
    got = np.concatenate([m["voxels"][:, None], m["s1"], m["s2"]], axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(bad), bad[:5].tolist())
    labels.close()


# ---- the serpentine at 128^3 ------------------------------------------------------------------------------------------

def test_serpentine_through_256_workgroups(built):
    """one piece, one voxel thick, through the key ranges of all 256 workgroups -- more than are resident at once"""
    vol, rec = cases.serpentine_case(128)
    xyz = np.argwhere(vol)
    volume = volume_of(vol)
    rng = np.random.default_rng(12)
    probe = np.concatenate([xyz[::7], rng.integers(0, 128, (50000, 3))]).astype(np.uint32)
    want = np.where(vol[tuple(probe.astype(np.int64).T)] != 0, 0, NONE).astype(np.uint32)
    for connectivity in (6, 26):
        labels = volume.labelComponents(connectivity)
        assert labels.count == 1
        assert labels.components().tobytes() == rec.tobytes(), connectivity
        assert np.array_equal(labels.at(probe), want), connectivity
        labels.close()
    volume.close()


# ---- 2. one box at 512^3 ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big(built):
    import cpuvoxelraycaster_amd as vrc
    src, dst = cases.big_scene(0), cases.big_scene(1)
    d_src, d_dst = apply(vrc.VoxelVolume(9), cases.big_edits(0)), apply(vrc.VoxelVolume(9), cases.big_edits(1))
    assert d_src.solidCount() == int(src.sum(dtype=np.int64)) and d_dst.solidCount() == int(dst.sum(dtype=np.int64))
    yield src, dst, d_src, d_dst
    d_src.close()
    d_dst.close()


@pytest.mark.parametrize("op", [cases.REPLACE, cases.OR])
@pytest.mark.parametrize("name", list(cases.COPIES))
def test_copy_region_at_512(big, name, op):
    """the whole-volume box and [1, 511)^3 from an odd offset: 4259840 words for 4194304 lanes; the control just below the cap"""
    src, dst, d_src, d_dst = big
    src_lo, size, dst_lo, second = cases.COPIES[name]
    lo, hi, _ = cases.copy_box(src_lo, size, dst_lo, 512, 512)
    assert cases.second_lanes(cases.box_word_items(lo, hi), cases.box_launch_groups(lo, hi) * cases.GROUP) == second
    work = d_dst.clone()
    work.copyRegion(d_src, src_lo, size, dst_lo, op)
    got = work.download()
    work.close()
    same(got, cases.copied(dst, src, src_lo, size, dst_lo, op), (name, op))


def test_stamp_identity_at_512_is_copy_region(big):
    """OR against the slices; REPLACE against copyRegion on the device, both ways, without a download"""
    import cpuvoxelraycaster_amd as vrc
    src, dst, d_src, d_dst = big
    S = 512
    identity = vrc.make_affine(*stamp_model.IDENTITY)
    work = d_dst.clone()
    work.stampAffine(d_src, identity, None, None, cases.OR)
    got = work.download()
    work.close()
    same(got, cases.copied(dst, src, (0, 0, 0), (S, S, S), (0, 0, 0), cases.OR), "identity OR")
    stamped, copied = d_dst.clone(), d_dst.clone()
    stamped.stampAffine(d_src, identity)
    copied.copyRegion(d_src, (0, 0, 0), (S, S, S), (0, 0, 0))
    assert stamped.solidCount() == copied.solidCount() == int(src.sum(dtype=np.int64))
    only = stamped.clone()
    only.copyRegion(copied, (0, 0, 0), (S, S, S), (0, 0, 0), cases.ANDNOT)          # stamped and not copied
    copied.copyRegion(stamped, (0, 0, 0), (S, S, S), (0, 0, 0), cases.ANDNOT)       # copied and not stamped
    assert only.solidCount() == 0 and copied.solidCount() == 0
    for v in (stamped, copied, only):
        v.close()


def test_quarter_turn_and_mirror_at_512(big):
    import cpuvoxelraycaster_amd as vrc
    src, dst, d_src, d_dst = big
    turned = d_src.transformed(vrc.affine_signed_permutation(*cases.TURN, 512))
    got = turned.download()
    turned.close()
    same(got, stamp_model.permuted(src, *cases.TURN), "turn")


def test_placed_stamp_at_512(big):
    """the source placed 3, -5 and 7 voxels off: a clipped box with odd bounds that still strides, OR into the destination"""
    src, dst, d_src, d_dst = big
    m, t, lo, hi, d = cases.placed_case()
    work = d_dst.clone()
    affine, got_lo, got_hi = work.stampPlaced(d_src, cases.IDENTITY_ROT, 1.0, cases.PLACED_PIVOTS[0], cases.PLACED_PIVOTS[1], cases.OR)
    got = work.download()
    work.close()
    assert list(affine.m) == list(m) and list(affine.t) == list(t) and list(got_lo) == lo and list(got_hi) == hi
    assert cases.box_word_items(lo, hi) > cases.BOX_GROUPS * cases.GROUP
    same(got, cases.shifted(dst, src, d, lo, hi, cases.OR), "placed")


# ---- 3. many boxes ------------------------------------------------------------------------------------------------------

def test_box_and_sphere_lists_where_a_lane_takes_several_words(built):
    """64^3: three boxes under 32 workgroups each (the whole-volume box: 9216 words for 8192 lanes), then 4100 under one
    workgroup each; fill, carve, count; the same with spheres"""
    import cpuvoxelraycaster_amd as vrc
    case = cases.many_box_case()
    S = 1 << cases.MANY_DEPTH
    for few, many, kind in ((case.few_boxes, case.many_boxes[:4100], "boxes"), (case.few_spheres, case.many_spheres, "spheres")):
        vol = cases.dense_of(case.base_edits, S)
        volume = apply(vrc.VoxelVolume(cases.MANY_DEPTH), case.base_edits)
        for items, solid in ((few, 1), (many, 0), (few[1:], 1)):
            apply(volume, [(kind, items, solid)])
            vol = cases.dense_of([("voxels", np.argwhere(vol), 1), (kind, items, solid)], S)
            same(volume.download(), vol, (kind, len(items), solid))
        assert 0 < int(vol.sum()) < S ** 3
        for boxes in (case.few_boxes, case.many_boxes):
            assert volume.countBoxes(boxes).tolist() == cases.count_boxes(vol, boxes), kind
        volume.close()
