"""The pair-contact calls without a GPU (include/vrc.h: vrc_rigid_pair_contacts, vrc_rigid_box_pair_count, vrc_rigid_box_pairs):
the numpy model of tests/pair_contact_model.py held against its own symmetries, against cases written out by hand and against
contact_model.contacts where the two rules agree, the cases of the GPU tests against what they claim, and every refusal that
is decided before the first HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

import components_model
import contact_model
import pair_contact_model as model
import rigid_model
import stamp_model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = (list(stamp_model.IDENTITY[0]), [0, 0, 0])


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


# ---- the model ---------------------------------------------------------------------------------------------------

def test_model_two_voxels_by_hand():
    """8^3: piece 0 is the voxel (3, 4, 5), piece 1 the voxel (5, 4, 5).  Moved together they touch, moved onto each other
    they overlap; on the volume's face there is no wall"""
    S = 8
    ids = np.full((S, S, S), model.NONE, np.uint32)
    ids[3, 4, 5], ids[5, 4, 5] = 0, 1
    apart = [IDENTITY, IDENTITY]
    assert model.pair_contacts(ids, apart, None, [(0, 1), (1, 0)], S) == [(1,) + model.ZERO[1:]] * 2
    # piece 1 moved by -1 along x: it sits at (4, 4, 5), the +x neighbour of piece 0.  For a = 0 the solid is at p + e_x:
    # n_x = 0 - 1 = -1, away from b; c = (7, 9, 11).  For a = 1, c = (9, 9, 11) and n_x = +1
    near = [IDENTITY] + rigid_model.translation_maps([[-1, 0, 0]])
    assert model.pair_contacts(ids, near, None, [(0, 1), (1, 0)], S) == [(1, 0, [0, 0, 0], [0, 0, 0], 1, [7, 9, 11], [-1, 0, 0]),
                                                                         (1, 0, [0, 0, 0], [0, 0, 0], 1, [9, 9, 11], [1, 0, 0])]
    onto = [IDENTITY] + rigid_model.translation_maps([[-2, 0, 0]])
    assert model.pair_contacts(ids, onto, None, [(0, 1)], S) == [(1, 1, [7, 9, 11], [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])]
    # in the corner of the volume and b far away: posed, and nothing else -- contact_model.contacts would see three walls
    corner = rigid_model.translation_maps([[-3, -4, -5]]) + [IDENTITY]
    assert model.pair_contacts(ids, corner, None, [(0, 1)], S) == [(1,) + model.ZERO[1:]]
    assert contact_model.contacts(ids, corner[:1], None, np.zeros((S, S, S), np.uint8))[0][4] == 1
    # skipped pieces: a skipped gives zero, b skipped leaves `posed`; an index beyond the pieces gives zero
    assert model.pair_contacts(ids, onto, None, [(0, 1), (1, 0)], S, keep=[0, 1]) == [model.ZERO, (1,) + model.ZERO[1:]]
    assert model.pair_contacts(ids, onto, [[0, 0, 0, 8, 8, 8], [4, 0, 0, 3, 8, 8]], [(0, 1), (1, 0)], S) == [(1,) + model.ZERO[1:], model.ZERO]
    assert model.pair_contacts(ids, onto, None, [(0, 2), (7, 0)], S) == [model.ZERO, model.ZERO]


def test_model_symmetry_and_the_self_pair():
    debris, ids, maps, boxes, keep, base = rigid_model.pose_case(32, 5)
    n = 12
    sets = contact_model.posed_sets(ids, maps[:n], boxes[:n], 32, keep[:n])
    records = dict(zip(all_pairs(n), model.records_of(sets, all_pairs(n), 32)))
    shown = 0
    for a in range(n):
        same = records[a, a]
        assert same[1] == same[0] and same[4] == 0 and same[6] == [0, 0, 0]   # overlap == posed, touch == 0
        for b in range(a):
            assert records[a, b][1] == records[b, a][1] and records[a, b][2] == records[b, a][2], (a, b)
            shown += records[a, b][1] > 0
    assert shown > 2


def test_model_equals_the_walled_model_away_from_the_faces():
    """for pieces kept one voxel away from the faces, pair (a, b) is contact_model.contacts of a against the dense placement
    of b: the two rules differ at the walls only"""
    vol, offsets = model.inner_blocks()
    ids, rec = components_model.label(vol, 6)
    maps = rigid_model.translation_maps(offsets)
    n = len(rec)
    got = model.pair_contacts(ids, maps, None, all_pairs(n), 32)
    for b in range(n):
        world = contact_model.posed(ids, b, maps[b], None, 32)
        want = contact_model.contacts(ids, maps, None, world)
        assert [got[a * n + b] for a in range(n)] == want, b
    assert sum(r[1] > 0 for r in got) > n and sum(r[4] > 0 for r in got) > 2


def test_model_box_pairs_by_hand_and_its_properties():
    S = 16
    boxes = np.array([[0, 0, 0, 4, 4, 4],
                      [4, 0, 0, 8, 4, 4],          # meets box 0 at a face
                      [4, 4, 0, 8, 8, 4],          # meets box 0 at an edge, box 1 at a face
                      [4, 4, 4, 8, 8, 8],          # meets box 0 at a corner
                      [9, 0, 0, 12, 4, 4],         # one voxel away from box 1: no candidate
                      [6, 6, 6, 6, 9, 9],          # empty
                      [9, 9, 9, 7, 12, 12],        # inverted
                      [14, 14, 14, 40, 40, 40],    # clipped
                      [16, 0, 0, 20, 4, 4]], np.uint32)      # wholly outside
    got = [tuple(p) for p in model.box_pairs(boxes, S).tolist()]
    assert got == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, 3), (3, 0), (3, 1), (3, 2)]
    assert [tuple(p) for p in model.box_pairs(boxes, S, keep=[1, 1, 0, 1, 1, 1, 1, 1, 1]).tolist()] == [(0, 1), (0, 3), (1, 0), (1, 3), (3, 0), (3, 1)]
    rng = np.random.default_rng(4)
    lo = rng.integers(0, 24, (40, 3))
    boxes = np.concatenate([lo, lo + rng.integers(-1, 15, (40, 3))], 1).astype(np.uint32)
    keep = (rng.random(40) < 0.8).astype(np.uint8)
    pairs = [tuple(p) for p in model.box_pairs(boxes, 32, keep).tolist()]
    assert len(pairs) > 30 and pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
    assert all((b, a) in set(pairs) and a != b for a, b in pairs)
    skipped = {i for i in range(40) if not keep[i] or model.clipped(boxes[i], 32) is None}
    assert len(skipped) > 5 and not skipped & {v for p in pairs for v in p}
    assert model.box_pairs(boxes[:1], 32).shape == (0, 2)


def test_model_cases_are_what_they_claim():
    for axis, sign in contact_model.DIRECTIONS:
        for overlap in (False, True):
            ids, maps, boxes, pairs, expected = model.bit_position_case(axis, sign, overlap)
            assert model.pair_contacts(ids, maps, boxes, pairs, 32) == expected       # the hand-written records are the model's
            assert len(pairs) == 32 and [tuple(p) for p in pairs.tolist()] == [tuple(p) for p in model.box_pairs(boxes, 32).tolist() if p[1] == p[0] + 32]
    vol = rigid_model.random_debris(16, 3)
    ids, rec, maps, boxes, keep = model.turned_case(vol, 6, 32, 3)
    pairs = model.box_pairs(boxes, 32, keep)
    records = model.pair_contacts(ids, maps, boxes, pairs, 32, keep)
    assert len(pairs) > 10 and sum(r[1] > 0 for r in records) > 2 and sum(r[4] > 0 for r in records) > 2
    assert sum(r[0] > 0 for r in records) > len(records) // 2


# ---- refusals ------------------------------------------------------------------------------------------------------

def fake_labels(count):
    """32 words that read as a vrc_labels on device 0 with `count` pieces (uint64 at byte 8) and nothing behind it"""
    words = (C.c_uint32 * 128)()
    words[2] = count
    return words


def test_pair_contact_refusals_need_no_gpu(built):
    """NULLs, a bad mem kind, a posed depth outside 2..10, too many pairs, a map beyond the limits and a pair index beyond the
    pieces are VRC_ERR_INVALID with the function's name before any HIP call: the handle here is no labels at all, and nothing
    is written"""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    what = b"vrc_rigid_pair_contacts: "
    none, two = fake_labels(0), fake_labels(2)
    p0, p2 = C.cast(none, C.c_void_p), C.cast(two, C.c_void_p)
    out = np.full(3, 9, capi.CONTACT_DTYPE)
    good = np.zeros(2, capi.AFFINE_DTYPE)
    good["m"][:] = IDENTITY[0]
    pairs = np.array([[0, 1], [1, 1], [1, 0]], np.uint32)
    call = L.vrc_rigid_pair_contacts
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert call(None, None, capi.ptr(good), None, 5, 3, capi.ptr(pairs), capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == what + b"null labels"
        assert call(p2, None, None, None, 5, 3, capi.ptr(pairs), capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == what + b"null maps with 2 components"
        assert call(p2, None, capi.ptr(good), None, 5, 3, None, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == what + b"null pairs with 3 pairs"
        assert call(p2, None, capi.ptr(good), None, 5, 3, capi.ptr(pairs), None, mem, None) == -1
        assert L.vrc_last_error() == what + b"null records with 3 pairs"
        assert call(p2, None, capi.ptr(good), None, 5, 1 << 32, capi.ptr(pairs), capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error().startswith(what + b"4294967296 pairs are too many")
        for depth in (0, 1, 11, 0xFFFFFFFF):
            assert call(p2, None, capi.ptr(good), None, depth, 3, capi.ptr(pairs), capi.ptr(out), mem, None) == -1
            assert L.vrc_last_error() == what + b"posed depth %d not in [2,10]" % depth
        # no pairs, or no pieces: legal without a device, nothing written
        assert call(p2, None, capi.ptr(good), None, 5, 0, None, None, mem, None) == 0
        assert call(p0, None, None, None, 5, 3, capi.ptr(pairs), capi.ptr(out), mem, None) == 0
    for mem in (-1, 2, 7):
        assert call(p2, None, capi.ptr(good), None, 5, 3, capi.ptr(pairs), capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == what + b"bad mem kind %d" % mem
    bad = good.copy()
    bad["m"][1][4] = (1 << 20) + 1
    assert call(p2, None, capi.ptr(bad), None, 5, 3, capi.ptr(pairs), capi.ptr(out), capi.VRC_MEM_HOST, None) == -1
    assert L.vrc_last_error() == what + b"piece 1: m[4] = 1048577 beyond +-2^20"
    for k, side, index in ((0, 1, 2), (2, 0, 7), (1, 1, 0xFFFFFFFF)):
        wrong = pairs.copy()
        wrong[k:, side] = index                                                 # the first bad pair is named
        assert call(p2, None, capi.ptr(good), None, 5, 3, capi.ptr(wrong), capi.ptr(out), capi.VRC_MEM_HOST, None) == -1
        assert L.vrc_last_error() == what + b"pair %d: piece %d of 2 components" % (k, index), L.vrc_last_error()
    assert out.tobytes() == np.full(3, 9, capi.CONTACT_DTYPE).tobytes()
    assert list(two) == [0, 0, 2] + [0] * 125 and not any(none)


def test_box_pair_refusals_need_no_gpu(built):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    none, two, many = fake_labels(0), fake_labels(2), fake_labels((1 << 20) + 1)
    p0, p2, pm = (C.cast(v, C.c_void_p) for v in (none, two, many))
    boxes = np.zeros((2, 6), np.uint32)
    pairs = np.full((4, 2), 9, np.uint32)
    count = C.c_uint64(77)
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        for what, call in ((b"vrc_rigid_box_pair_count: ", lambda l, b, d, m: L.vrc_rigid_box_pair_count(l, None, b, d, C.byref(count), m, None)),
                           (b"vrc_rigid_box_pairs: ", lambda l, b, d, m: L.vrc_rigid_box_pairs(l, None, b, d, 0, 4, capi.ptr(pairs), m, None))):
            assert call(None, capi.ptr(boxes), 5, mem) == -1 and L.vrc_last_error() == what + b"null labels"
            assert call(p2, None, 5, mem) == -1 and L.vrc_last_error() == what + b"null boxes with 2 components"
            assert call(pm, capi.ptr(boxes), 5, mem) == -1 and L.vrc_last_error().startswith(what + b"1048577 components are too many")
            for depth in (1, 11):
                assert call(p2, capi.ptr(boxes), depth, mem) == -1 and L.vrc_last_error() == what + b"posed depth %d not in [2,10]" % depth
            assert call(p2, capi.ptr(boxes), 5, 3) == -1 and L.vrc_last_error() == what + b"bad mem kind 3"
            assert call(p0, None, 5, mem) == 0                                  # no pieces: no pairs, no device
        assert L.vrc_rigid_box_pair_count(p2, None, capi.ptr(boxes), 5, None, mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_box_pair_count: null count"
        assert L.vrc_rigid_box_pairs(p2, None, capi.ptr(boxes), 5, 0, 4, None, mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_box_pairs: null buffer with capacity 4"
        assert L.vrc_rigid_box_pairs(p2, None, capi.ptr(boxes), 5, 0, 0, None, mem, None) == 0       # capacity 0 with NULL pairs
    assert count.value == 0 and (pairs == 9).all()                              # the count of no pieces is 0; no pair was written


def test_python_arguments(built):
    import cpuvoxelraycaster_amd as vrc
    labels = vrc.VoxelLabels(None, 2, 4, 0)
    two = np.zeros(2, vrc.capi.AFFINE_DTYPE)
    with pytest.raises(ValueError, match="maps"):
        labels.pairContacts(np.zeros(3, vrc.capi.AFFINE_DTYPE), [[0, 1]])
    with pytest.raises(ValueError, match="boxes"):
        labels.pairContacts(two, [[0, 1]], boxes=np.zeros((1, 6), np.uint32))
    with pytest.raises(ValueError, match="keep"):
        labels.pairContacts(two, [[0, 1]], keep=[1])
    with pytest.raises(ValueError, match="needs boxes"):
        labels.pairContacts(two)
    with pytest.raises(ValueError, match="boxes"):
        labels.candidatePairs(np.zeros((3, 6), np.uint32))
    with pytest.raises(ValueError, match="keep"):
        labels.candidatePairs(np.zeros((2, 6), np.uint32), keep=[1, 1, 1])


def test_host_adapter_with_pair_contacts_compiles(built):
    """HipVoxelLabels::candidatePairs / pairContacts in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelLabels& labels, const std::vector<vrc_affine>& maps) {\n'
           '    std::vector<uint32_t> boxes(6 * labels.count(), 0u);\n'
           '    std::vector<uint8_t> keep(labels.count(), 1);\n'
           '    std::vector<uint32_t> pairs = labels.candidatePairs(boxes, 5), fewer = labels.candidatePairs(boxes, 5, &keep);\n'
           '    std::vector<vrc_piece_contact> all = labels.pairContacts(maps, pairs, 5);\n'
           '    std::vector<vrc_piece_contact> some = labels.pairContacts(maps, fewer, 5, &boxes, &keep);\n'
           '    return all[0].overlap + some[0].touch;\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
