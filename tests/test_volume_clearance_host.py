"""vrc_rigid_clearance without a GPU: the numpy model (tests/clearance_model.py) against records written out by hand, the rule of
VoxelLabels.freeRadius, the cases of the GPU tests held to what they claim, the record's layout, the refusals that are decided
before the first HIP call, and the C++ adapter's syntax."""
import ctypes as C
import os

import numpy as np
import pytest

import clearance_model as model
import components_model
import contact_model
import distance_model
import posed_cases
import rigid_model
import stamp_model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = model.NONE
IDENTITY = (list(stamp_model.IDENTITY[0]), [0, 0, 0])


# ---- the model -----------------------------------------------------------------------------------------------------

def test_model_two_voxels_and_three_values_by_hand():
    """a two-voxel piece over a field of 4^3 that holds 9 everywhere but for a 4, a 25 and a NONE"""
    D = np.full((4, 4, 4), 9, np.uint32)
    D[1, 2, 3], D[3, 0, 0], D[2, 2, 2] = 4, 25, NONE
    assert model.record([[1, 2, 3], [3, 0, 0]], D) == (2, 0, 29, 4, [1, 2, 3], 25, [3, 0, 0])
    # a tie: both hold 9, the smaller dense index (1*4 + 0)*4 + 2 = 18 < (1*4 + 1)*4 + 0 = 20 wins for the minimum AND the maximum
    assert model.record([[1, 1, 0], [1, 0, 2]], D) == (2, 0, 18, 9, [1, 0, 2], 9, [1, 0, 2])
    # a NONE is counted and takes part in nothing else
    assert model.record([[2, 2, 2], [3, 0, 0]], D) == (2, 1, 25, 25, [3, 0, 0], 25, [3, 0, 0])
    assert model.record([[2, 2, 2]], D) == (1, 1, 0, NONE, [0, 0, 0], 0, [0, 0, 0])
    assert model.record([], D) == model.EMPTY == (0, 0, 0, NONE, [0, 0, 0], 0, [0, 0, 0])
    # a value of 0 at a voxel: found as the minimum, and as the maximum where it is all there is
    D[0, 0, 1] = 0
    assert model.record([[0, 0, 1]], D) == (1, 0, 0, 0, [0, 0, 1], 0, [0, 0, 1])


def test_model_through_a_map_by_hand():
    """the two-voxel piece (1, 1, 1), (1, 1, 2) of an 8^3 labelling, moved by (2, 0, -1) into a field of 8^3 = the squared
    distance to the single solid voxel (3, 4, 1): the posed voxels (3, 1, 0) and (3, 1, 1) hold 10 and 9"""
    vol = np.zeros((8, 8, 8), np.uint8)
    vol[1, 1, 1:3] = 1
    ids, rec = components_model.label(vol, 6)
    world = np.zeros((8, 8, 8), np.uint8)
    world[3, 4, 1] = 1
    D = distance_model.field(world)
    maps = rigid_model.translation_maps([[2, 0, -1]])
    assert model.clearance(ids, maps, None, D) == [(2, 0, 19, 9, [3, 1, 1], 10, [3, 1, 0])]
    assert model.clearance(ids, maps, [[0, 0, 0, 8, 8, 1]], D) == [(1, 0, 10, 10, [3, 1, 0], 10, [3, 1, 0])]     # the box cuts z = 1 off
    assert model.clearance(ids, maps, [[4, 4, 4, 4, 8, 8]], D) == [model.EMPTY]
    assert model.clearance(ids, maps, None, D, [0]) == [model.EMPTY]
    beyond = [([(1 << 20) + 1] + IDENTITY[0][1:], [0, 0, 0])]
    assert model.clearance(ids, beyond, None, D) == [model.EMPTY]
    # the posed set is contact_model's
    assert np.array_equal(np.argwhere(contact_model.posed(ids, 0, maps[0], None, 8)), posed_cases.posed_points(ids, 0, maps[0], None, 8))


def test_free_radius_rule(built):
    """min_value 0: the piece overlaps, -1; 1: any step may hit, 0; 2, 4: one voxel (1 < 2, 1 < 4, but 4 is not below 4); 5: two;
    NONE: nothing to hit, the field's S.  The library's isqrt form against the definition by counting up"""
    import cpuvoxelraycaster_amd as vrc
    values = [0, 1, 2, 4, 5, NONE]
    assert vrc.free_radius(values, 32).tolist() == [-1, 0, 1, 1, 2, 32]
    assert vrc.free_radius(values, 32).dtype == np.int64
    more = list(range(0, 300)) + [3 * 1023 ** 2, (1 << 30) - 1, NONE]
    assert vrc.free_radius(more, 1024).tolist() == [model.free_radius(v, 1024) for v in more]


def test_translated_map_moves_the_posed_set():
    """the map of the advancement rounds: the posed set under translated(mp, o) is the posed set under mp, moved by o"""
    case = model.advancement_case(3)
    shown = 0
    for i in range(0, len(case.maps), 7):
        o = case.rounds[0][i]
        moved = posed_cases.posed_points(case.ids, i, model.translated(case.maps[i], o), None, 64)
        assert np.array_equal(moved, case.points[i] + o)
        shown += len(moved) > 0
    assert shown > 5


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [3, 4])
def test_advancement_case_is_what_it_claims(seed):
    case = model.advancement_case(seed)
    everything = np.concatenate(case.points)
    assert everything.min() >= 16 and everything.max() < 48                   # nothing is clipped, no piece left out by a box
    assert 0 < case.world[12:52, 12:52, 12:52].sum() <= 48 and case.world[:12].any() and case.world[52:].any()
    posed = np.array([r[0] for r in case.records])
    least = np.array([r[3] for r in case.records], np.int64)
    assert (posed > 0).sum() > 40
    for o in case.rounds:
        assert np.abs(o).max() <= model.REACH
        inside = ((o ** 2).sum(1) < least) & (posed > 0)
        assert inside.sum() > 10 and (~inside & (posed > 0)).sum() > 10       # both sides of |o|^2 < min_value
    assert 2 * case.reach.sum() >= len(case.records)                          # the sharp round reaches at least half the pieces
    for i in np.flatnonzero(case.reach):
        q = np.array(case.records[i][4]) + case.last[i]
        assert case.world[tuple(q)] == 1 and int((case.last[i] ** 2).sum()) == case.records[i][3]
    # the model itself obeys the bound it is used to test: a translation within it meets no solid voxel
    for i in np.flatnonzero(posed > 0)[::9]:
        o = case.rounds[0][i]
        hit = case.world[tuple((case.points[i] + o).T)].any()
        assert not (hit and int((o ** 2).sum()) < least[i])


def test_plate_case_is_what_it_claims():
    plate, world, maps, box = model.plate_case()
    ids, rec = components_model.label(plate, 6)
    assert len(rec) == 1
    D = distance_model.field(world)
    gx, gy = posed_cases.posed_grid(1, 64)
    flat = posed_cases.posed_points(ids, 0, maps[0], box, 64)
    assert len(flat) == 1600 and model.record(flat, D) == (1600, 0, 1600 * 324, 324, [10, 20, 12], 324, [10, 20, 12])
    tilted = posed_cases.posed_points(ids, 0, maps[1], box, 64)
    r = model.record(tilted, D)
    values = D[tuple(tilted.T)]
    lowest = tilted[values == r[3]]
    assert len(lowest) == 40 and len(set(lowest[:, 0].tolist())) == 1 and len(set(lowest[:, 1].tolist())) == 1     # one row along z
    assert r[4] == [int(v) for v in lowest[np.argmin(lowest[:, 2])]] and r[4][0] > r[6][0] and (values == r[5]).sum() > 1
    for points in (flat, tilted):
        counts = posed_cases.item_counts(points, box, 64)
        assert len(counts) <= gx * posed_cases.GROUP                          # a lane has one item: workgroup = item // GROUP
        groups = set((np.flatnonzero(counts) // posed_cases.GROUP).tolist())
        waves = set((np.flatnonzero(counts) // 64).tolist())
        assert len(groups) > 3 and len(waves) > len(groups)


def test_small_world_cases_pose_every_piece():
    for S in (4, 8):
        debris, maps, boxes = model.small_world_case(S)
        ids, rec = components_model.label(debris, 6)
        assert len(rec) == 3
        for bx in (boxes, None):
            sets = posed_cases.posed_point_sets(ids, maps, bx, S)
            assert all(len(p) > 1 for p in sets)
    # 4^3: the pieces have voxels in both occupancy words and in both halves of each (the four brick rows 2 cx + cy)
    debris, maps, boxes = model.small_world_case(4)
    ids, _ = components_model.label(debris, 6)
    p = np.concatenate(posed_cases.posed_point_sets(ids, maps, None, 4))
    rows = set((((p[:, 0] >> 1) * 2 + (p[:, 1] >> 1))).tolist())
    assert rows == {0, 1, 2, 3}


def test_fields_hold_what_the_random_test_needs():
    _, _, _, _, _, base = rigid_model.pose_case(32, 5)
    fields = model.fields_of(base)
    assert [name for name, _, _ in fields] == ["solid", "solid, open border", "empty", "travel"]
    travel = fields[3][2]
    assert (travel == NONE).sum() > 1000 and (travel != NONE).sum() > 1000
    assert all((D != NONE).all() for _, _, D in fields[:3])


# ---- the record and the refusals -----------------------------------------------------------------------------------

def test_struct_layout(built):
    from cpuvoxelraycaster_amd import capi
    names = ("posed", "none", "sum", "min_value", "min_at", "max_value", "max_at", "reserved")
    assert capi.CLEARANCE_DTYPE.itemsize == 64
    assert [capi.CLEARANCE_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 24, 28, 40, 44, 56]
    src = ('#include "%s"\n#include <stddef.h>\n'
           'static_assert(sizeof(vrc_piece_clearance) == 64 && offsetof(vrc_piece_clearance, sum) == 16 && offsetof(vrc_piece_clearance, min_value) == 24 &&'
           ' offsetof(vrc_piece_clearance, min_at) == 28 && offsetof(vrc_piece_clearance, max_value) == 40 && offsetof(vrc_piece_clearance, max_at) == 44 &&'
           ' offsetof(vrc_piece_clearance, reserved) == 56, "clearance");\n') % os.path.join(ROOT, "include", "vrc.h")
    check_cpp_syntax(src)


def test_clearance_refusals_need_no_gpu(built):
    """NULLs, a bad mem kind, a device mismatch and maps beyond the limits are VRC_ERR_INVALID with the function's name before
    any HIP call: the handles here are not labels or fields at all, and nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b, c, one = (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)()
    for i in range(128):
        c[i] = 0x01010101                                                     # every field differs
    one[2] = 1                                                                # labels: device 0, depth 0, count 1 (uint64 at byte 8)
    pa, pb, pc, p1 = (C.cast(v, C.c_void_p) for v in (a, b, c, one))
    out = np.full(2, 9, capi.CLEARANCE_DTYPE)
    good = np.zeros(1, capi.AFFINE_DTYPE)
    good["m"][0] = IDENTITY[0]
    name = b"vrc_rigid_clearance: "
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_rigid_clearance(None, None, capi.ptr(good), None, pb, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == name + b"null argument"
        assert L.vrc_rigid_clearance(pa, None, capi.ptr(good), None, None, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == name + b"null argument"
        assert L.vrc_rigid_clearance(pa, None, capi.ptr(good), None, pc, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == name + b"labels on device 0, field on device 16843009"
        assert L.vrc_rigid_clearance(p1, None, None, None, pb, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == name + b"null maps with 1 components"
        assert L.vrc_rigid_clearance(p1, None, capi.ptr(good), None, pb, None, mem, None) == -1
        assert L.vrc_last_error() == name + b"null records with 1 components"
    for mem in (-1, 2, 7):
        assert L.vrc_rigid_clearance(pa, None, capi.ptr(good), None, pb, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == name + b"bad mem kind %d" % mem
    limit_m, limit_t = 1 << 20, 1 << 40
    for field, index, value, text in (("reserved", None, 1, b"piece 0: reserved is 1, not 0"),
                                      ("m", 0, limit_m + 1, b"piece 0: m[0] = 1048577 beyond +-2^20"),
                                      ("t", 2, -limit_t - 1, b"piece 0: t[2] = -1099511627777 beyond +-2^40")):
        bad = good.copy()
        if index is None:
            bad[field][0] = value
        else:
            bad[field][0][index] = value
        assert L.vrc_rigid_clearance(p1, None, capi.ptr(bad), None, pb, capi.ptr(out), capi.VRC_MEM_HOST, None) == -1
        assert L.vrc_last_error() == name + text, L.vrc_last_error()
    # no pieces: legal without a device, nothing written
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_rigid_clearance(pa, None, None, None, pb, None, mem, None) == 0
    assert out.tobytes() == np.full(2, 9, capi.CLEARANCE_DTYPE).tobytes()
    assert not any(a) and not any(b) and all(v == 0x01010101 for v in c) and list(one) == [0, 0, 1] + [0] * 125


def test_python_arguments(built):
    import cpuvoxelraycaster_amd as vrc
    labels = vrc.VoxelLabels(None, 2, 4, 0)
    two = np.zeros(2, vrc.capi.AFFINE_DTYPE)
    with pytest.raises(ValueError, match="maps"):
        labels.clearance(np.zeros(3, vrc.capi.AFFINE_DTYPE), None)
    with pytest.raises(ValueError, match="boxes"):
        labels.clearance(two, None, boxes=np.zeros((1, 6), np.uint32))
    with pytest.raises(ValueError, match="keep"):
        labels.freeRadius(two, None, keep=[1])


def test_host_adapter_with_clearance_compiles(built):
    """HipVoxelLabels::clearance in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelDistance& field, vrc_host::HipVoxelLabels& labels, const std::vector<vrc_affine>& maps) {\n'
           '    std::vector<uint32_t> boxes(6 * labels.count(), 0u);\n'
           '    std::vector<uint8_t> keep(labels.count(), 1);\n'
           '    std::vector<vrc_piece_clearance> all = labels.clearance(maps, field);\n'
           '    std::vector<vrc_piece_clearance> some = labels.clearance(maps, field, &boxes, &keep);\n'
           '    return all[0].posed + some[0].min_value;\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
