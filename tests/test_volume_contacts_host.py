"""The contact call without a GPU (include/vrc.h: vrc_rigid_contacts): the numpy model of tests/contact_model.py held against
cases written out by hand and against rigid_model.place_affine, the cases of the GPU tests against what they claim, the
record's layout, every refusal that is decided before the first HIP call, and the arithmetic of contact_properties."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import components_model
import contact_model as model
import fall_model
import rigid_model
import stamp_model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = model.NONE
IDENTITY = (list(stamp_model.IDENTITY[0]), [0, 0, 0])


# ---- the model ---------------------------------------------------------------------------------------------------

def cube_on_slab():
    """16^3: a slab y < 4 as the world, a 4 x 4 x 4 cube at x 5..8, y 8..11, z 6..9 as the one piece"""
    S = 16
    world = np.zeros((S, S, S), np.uint8)
    world[:, 0:4, :] = 1
    ids = np.full((S, S, S), NONE, np.uint32)
    ids[5:9, 8:12, 6:10] = 0
    return S, world, ids


def test_model_cube_resting_on_a_slab_by_hand():
    S, world, ids = cube_on_slab()
    # lowered by 4: the cube's lowest layer y = 4 stands on the slab's top layer y = 3.  16 voxels touch, each with the normal
    # +y (away from the slab).  Their c: x in 5..8 -> 11+13+15+17 = 56, four times each = 224; y = 4 -> 9 * 16 = 144;
    # z in 6..9 -> 13+15+17+19 = 64, four times = 256
    rest = rigid_model.translation_maps([[0, -4, 0]])
    assert model.contacts(ids, rest, None, world) == [(64, 0, [0, 0, 0], [0, 0, 0], 16, [224, 144, 256], [0, 16, 0])]
    # lowered one cell more: the lowest layer, now y = 3, is inside the slab; below it is slab, above it the cube's own next
    # layer, which is no part of the world: the 16 voxels have solid at y - 1 and open at y + 1, x and z neighbours solid on
    # both sides.  Layer y = 4 now touches.  c_y = 7 -> 112
    sunk = rigid_model.translation_maps([[0, -5, 0]])
    assert model.contacts(ids, sunk, None, world) == [(64, 16, [224, 112, 256], [0, 16, 0], 16, [224, 144, 256], [0, 16, 0])]
    # a quarter turn about y, q = (p_z, p_y, 15 - p_x): the cube lands on x 6..9, z 5..8 -- the same counts, the same y terms,
    # and c_x: 13+15+17+19 = 64, four times = 256, c_z: 224
    m, t = stamp_model.signed_permutation((2, 1, 0), (0, 0, 1), S)
    t = [t[0], t[1] + (4 << 17), t[2]]                                       # and lowered by 4: q_y = p_y + 4
    got = model.contacts(ids, [(m, t)], None, world)[0]
    assert got == (64, 0, [0, 0, 0], [0, 0, 0], 16, [256, 144, 224], [0, 16, 0])
    # skipped pieces: keep == 0, an empty box, a map beyond the limits
    assert model.contacts(ids, rest, None, world, keep=[0]) == [model.ZERO]
    assert model.contacts(ids, rest, [[3, 3, 3, 3, 9, 9]], world) == [model.ZERO]
    assert model.contacts(ids, [(rest[0][0], [1 << 41, 0, 0])], None, world) == [model.ZERO]


def test_model_corner_voxel_over_an_empty_world_by_hand():
    """one voxel posed at (0, 0, 0) of an empty 8^3 world: it touches three walls, the normal points into the volume; at
    (7, 7, 7) the other three"""
    S = 8
    ids = np.full((S, S, S), NONE, np.uint32)
    ids[3, 4, 5] = 0
    world = np.zeros((S, S, S), np.uint8)
    assert model.contacts(ids, rigid_model.translation_maps([[-3, -4, -5]]), None, world) == [(1, 0, [0, 0, 0], [0, 0, 0], 1, [1, 1, 1], [1, 1, 1])]
    assert model.contacts(ids, rigid_model.translation_maps([[4, 3, 2]]), None, world) == [(1, 0, [0, 0, 0], [0, 0, 0], 1, [15, 15, 15], [-1, -1, -1])]
    assert model.contacts(ids, [IDENTITY], None, world) == [(1, 0, [0, 0, 0], [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])]       # in the open: nothing
    # against itself as the world nothing is excluded: the voxel overlaps itself, no neighbour is solid
    assert model.contacts(ids, [IDENTITY], None, (ids == 0).astype(np.uint8)) == [(1, 1, [7, 9, 11], [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])]


def test_model_posed_set_is_place_affine_of_the_piece_alone():
    debris, ids, maps, boxes, keep, base = rigid_model.pose_case(32, 5)
    zeros = np.zeros_like(base)
    for i in range(0, len(maps), 3):
        alone = rigid_model.place_affine(ids, maps, boxes, zeros, rigid_model.OR, [j == i for j in range(len(maps))])
        assert np.array_equal(model.posed(ids, i, maps[i], boxes[i], 32), alone), i
    records = model.contacts(ids, maps, boxes, base, keep)
    assert all(rec == model.ZERO for rec, k in zip(records, keep) if not k)
    assert records[5] == records[6] == model.ZERO                             # the empty and the inverted box
    assert sum(rec[1] > 0 for rec in records) > 10 and sum(rec[4] > 0 for rec in records) > 10


def test_model_cases_are_what_they_claim():
    for axis, sign in model.DIRECTIONS:
        ids, targets, maps, boxes, world, expected = model.bit_position_case(axis, sign)
        assert sorted((int(p[0]) & 1) + 2 * (int(p[1]) & 1) + 4 * (int(p[2]) & 7) for p in targets[:32]) == list(range(32))
        assert model.contacts(ids, maps, boxes, world) == expected            # the hand-written records are the model's
        crossing = [p for p in targets if (p + model.AXES[axis] * sign)[axis] // (8 if axis == 2 else 2) != p[axis] // (8 if axis == 2 else 2)]
        assert crossing and len(crossing) < 64                                # obstacles in the same word and in the next one
    vol, offsets = model.wall_case()
    ids, rec = components_model.label(vol, 6)
    got = model.contacts(ids, rigid_model.translation_maps(offsets), None, np.zeros_like(vol))
    for k in range(6):
        n = [0, 0, 0]
        n[k >> 1] = 9 if k & 1 == 0 else -9
        assert (got[k][0], got[k][1], got[k][4], got[k][6]) == (27, 0, 9, n), k
    assert (got[6][4], got[6][6]) == (19, [9, 9, 9])                          # the corner: 27 - 8 voxels touch a face
    assert got[7][0] == 18 and got[7][4] == 9                                 # one layer beyond the volume: dropped
    # the end-to-end scene: nothing overlaps on entry, and nothing after the fall
    vol, supported, debris = model.end_to_end_case()
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 2 and not (debris & supported).any()
    offsets = fall_model.offsets_of(fall_model.drops(ids, supported, 2), 2)
    assert (offsets[:, 1] < 0).all()
    after = model.contacts(ids, rigid_model.translation_maps(offsets), rigid_model.moved_boxes(rec, offsets, 32), supported)
    assert all(r[1] == 0 and r[4] > 0 and r[6][1] > 0 for r in after)
    for name, world in model.worlds(16, 3):
        assert 0 < world.sum() < world.size, name


# ---- the record ----------------------------------------------------------------------------------------------------

def test_struct_layout(built):
    from cpuvoxelraycaster_amd import capi
    names = ("posed", "overlap", "overlap_s1", "overlap_n", "touch", "touch_s1", "touch_n", "reserved")
    assert capi.CONTACT_DTYPE.itemsize == 128 == C.sizeof(capi.PieceContact)
    assert [capi.CONTACT_DTYPE.fields[f][1] for f in names] == [getattr(capi.PieceContact, f).offset for f in names] == [0, 8, 16, 40, 64, 72, 96, 120]
    assert capi.CONTACT_DTYPE["overlap_n"].base == np.dtype("<i8") and capi.CONTACT_DTYPE["touch_s1"].base == np.dtype("<u8")
    src = ('#include "%s"\n#include <stddef.h>\n'
           'static_assert(sizeof(vrc_piece_contact) == 128 && offsetof(vrc_piece_contact, overlap_s1) == 16 && offsetof(vrc_piece_contact, overlap_n) == 40 &&'
           ' offsetof(vrc_piece_contact, touch) == 64 && offsetof(vrc_piece_contact, touch_n) == 96 && offsetof(vrc_piece_contact, reserved) == 120, "contact");\n'
           ) % os.path.join(ROOT, "include", "vrc.h")
    check_cpp_syntax(src)


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_contact_refusals_need_no_gpu(built):
    """NULLs, a bad mem kind, a device mismatch and maps beyond the limits are VRC_ERR_INVALID with the function's name before
    any HIP call: the handles here are not volumes or labels at all, and nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b, c, one = (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)()
    for i in range(128):
        c[i] = 0x01010101                                                     # every field differs, and as labels C > 0
    one[2] = 1                                                                # labels: device 0, depth 0, count 1 (uint64 at byte 8)
    pa, pb, pc, p1 = (C.cast(v, C.c_void_p) for v in (a, b, c, one))
    out = np.full(2, 9, capi.CONTACT_DTYPE)
    good = np.zeros(1, capi.AFFINE_DTYPE)
    good["m"][0] = IDENTITY[0]
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_rigid_contacts(None, None, capi.ptr(good), None, pb, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_contacts: null argument"
        assert L.vrc_rigid_contacts(pa, None, capi.ptr(good), None, None, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_contacts: null argument"
        assert L.vrc_rigid_contacts(pa, None, capi.ptr(good), None, pc, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_contacts: labels on device 0, volume on device 16843009"
        assert L.vrc_rigid_contacts(p1, None, None, None, pb, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_contacts: null maps with 1 components"
        assert L.vrc_rigid_contacts(p1, None, capi.ptr(good), None, pb, None, mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_contacts: null records with 1 components"
    for mem in (-1, 2, 7):
        assert L.vrc_rigid_contacts(pa, None, capi.ptr(good), None, pb, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_contacts: bad mem kind %d" % mem
    limit_m, limit_t = 1 << 20, 1 << 40
    for field, index, value, text in (("reserved", None, 1, b"piece 0: reserved is 1, not 0"),
                                      ("m", 0, limit_m + 1, b"piece 0: m[0] = 1048577 beyond +-2^20"),
                                      ("m", 8, -limit_m - 1, b"piece 0: m[8] = -1048577 beyond +-2^20"),
                                      ("t", 0, limit_t + 1, b"piece 0: t[0] = 1099511627777 beyond +-2^40"),
                                      ("t", 2, -limit_t - 1, b"piece 0: t[2] = -1099511627777 beyond +-2^40")):
        bad = good.copy()
        if index is None:
            bad[field][0] = value
        else:
            bad[field][0][index] = value
        assert L.vrc_rigid_contacts(p1, None, capi.ptr(bad), None, pb, capi.ptr(out), capi.VRC_MEM_HOST, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_contacts: " + text, L.vrc_last_error()
    # no pieces: legal without a device, nothing written
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_rigid_contacts(pa, None, None, None, pb, None, mem, None) == 0
    assert out.tobytes() == np.full(2, 9, capi.CONTACT_DTYPE).tobytes()
    assert not any(a) and not any(b) and all(v == 0x01010101 for v in c) and list(one) == [0, 0, 1] + [0] * 125


def test_python_arguments(built):
    import cpuvoxelraycaster_amd as vrc
    labels = vrc.VoxelLabels(None, 2, 4, 0)
    two = np.zeros(2, vrc.capi.AFFINE_DTYPE)
    with pytest.raises(ValueError, match="maps"):
        labels.contacts(np.zeros(3, vrc.capi.AFFINE_DTYPE), None)
    with pytest.raises(ValueError, match="boxes"):
        labels.contacts(two, None, boxes=np.zeros((1, 6), np.uint32))
    with pytest.raises(ValueError, match="keep"):
        labels.collides(two, None, keep=[1])


def test_host_adapter_with_contacts_compiles(built):
    """HipVoxelLabels::contacts in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelLabels& labels, const std::vector<vrc_affine>& maps) {\n'
           '    std::vector<uint32_t> boxes(6 * labels.count(), 0u);\n'
           '    std::vector<uint8_t> keep(labels.count(), 1);\n'
           '    std::vector<vrc_piece_contact> all = labels.contacts(maps, world);\n'
           '    std::vector<vrc_piece_contact> some = labels.contacts(maps, world, &boxes, &keep);\n'
           '    return all[0].overlap + some[0].touch;\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)


# ---- contact_properties --------------------------------------------------------------------------------------------

def test_contact_properties_within_one_unit_in_the_last_place(built):
    import cpuvoxelraycaster_amd as vrc
    cases = [(64, 16, [224, 112, 256], [0, 16, 0], 16, [224, 144, 256], [0, 16, 0]),
             (5, 3, [7, 9, 11], [1, -2, 2], 2, [1001, 77, 3], [-1, 1, 0]),
             (1 << 30, 1 << 29, [(1 << 40) + 12345, (1 << 39) + 1, 3 << 38], [(1 << 29) - 1, -(1 << 28) - 7, 12345],
              1 << 20, [(1 << 30) + 1, (1 << 31) - 1, 1 << 20], [-(1 << 20), 1 << 19, -3]),
             (9, 0, [0, 0, 0], [0, 0, 0], 4, [10, 20, 30], [0, 0, 0]),           # a count without a direction
             model.ZERO]
    rec = np.zeros(len(cases), vrc.capi.CONTACT_DTYPE)
    for i, case in enumerate(cases):
        rec[i] = case + (0,)
    got = vrc.contact_properties(rec)
    assert len(got) == 4 and all(g.dtype == np.float64 and g.shape == (len(cases), 3) for g in got)
    for i, case in enumerate(cases):
        for g, exact in zip(got, model.contact_properties(case)):
            for value, want in zip(g[i].tolist(), exact):
                assert abs(Fraction(value) - want) <= abs(want) * Fraction(1, 1 << 52), (i, value, float(want))
    assert got[0][0].tolist() == [7.0, 3.5, 8.0] and got[1][0].tolist() == [0.0, 1.0, 0.0] and got[2][0].tolist() == [7.0, 4.5, 8.0]
    assert got[1][1].tolist() == [1 / 3, -2 / 3, 2 / 3]
    assert not got[0][4].any() and not got[1][4].any() and not got[2][4].any() and not got[3][4].any() and not got[3][3].any()
