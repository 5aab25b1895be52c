"""The rigid-piece calls without a GPU (include/vrc.h: vrc_rigid_moments, vrc_rigid_place_affine, vrc_affine_place_box): the
numpy model of tests/rigid_model.py held against cases written out by hand and against the fall model, the host helper
against vrc_affine_place and the model, every refusal that is decided before the first HIP call, and the arithmetic of
mass_properties against exact fractions."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import components_model
import fall_model
import rigid_model as model
import stamp_model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = model.NONE


# ---- the model ---------------------------------------------------------------------------------------------------

def test_model_moments_by_hand():
    """4^3: piece 0 = the voxels (0,0,0) and (1,0,0); piece 1 = the single voxel (3,2,1)"""
    ids = np.full((4, 4, 4), NONE, np.uint32)
    ids[0, 0, 0] = ids[1, 0, 0] = 0
    ids[3, 2, 1] = 1
    # piece 0: c = (1,1,1) and (3,1,1): s1 = (4,2,2); xx = 1+9, yy = zz = 2, xy = xz = 1+3, yz = 2
    # piece 1: c = (7,5,3): s2 = 49, 25, 9, 35, 21, 15
    want = [(2, [4, 2, 2], [10, 2, 2, 4, 4, 2]), (1, [7, 5, 3], [49, 25, 9, 35, 21, 15])]
    assert model.moments(ids) == want
    assert model.moments_fast(ids, 2) == want
    # the two voxels of piece 0: centre (1, 0.5, 0.5); about it the point masses give sum r_x^2 = 0.5, so
    # I_xx = 0 + 2/6, I_yy = I_zz = 0.5 + 2/6, no products
    mass, centre, inertia = model.mass_properties(*want[0])
    assert mass == 2 and centre == [1, Fraction(1, 2), Fraction(1, 2)]
    assert inertia == [[Fraction(1, 3), 0, 0], [0, Fraction(5, 6), 0], [0, 0, Fraction(5, 6)]]
    # one voxel: the unit cube's own tensor
    assert model.mass_properties(*want[1])[2] == [[Fraction(1, 6), 0, 0], [0, Fraction(1, 6), 0], [0, 0, Fraction(1, 6)]]


def test_model_closed_form_of_a_full_cube():
    for S in (4, 8, 16):
        ids = np.zeros((S, S, S), np.uint32)
        assert model.moments_fast(ids, 1) == [model.solid_cube_moments(S)]
    n, s1, s2 = model.solid_cube_moments(32)
    assert s1 == [n * 32] * 3
    assert model.solid_cube_moments(64)[2][0] < 1 << 32 < model.solid_cube_moments(128)[2][0]      # why the GPU test goes to 128^3
    # a solid cube of side S: I = n (S^2 / 6), the textbook value, about its centre
    mass, centre, inertia = model.mass_properties(*model.solid_cube_moments(8))
    assert centre == [4, 4, 4] and inertia[0][0] == Fraction(512 * 64, 6) and inertia[0][1] == 0


def test_model_placement_with_translations_is_the_fall_place():
    for S, connectivity, direction, limit, seed in fall_model.RANDOM_CASES[::5]:
        debris, fixed = fall_model.random_case(S, seed)
        ids, rec = components_model.label(debris, connectivity)
        rng = np.random.default_rng(seed)
        offsets = rng.integers(-S // 2, S // 2 + 1, (len(rec), 3))
        keep = (rng.random(len(rec)) < 0.7).astype(np.uint8)
        maps = model.translation_maps(offsets)
        for op_or in (True, False):
            want = fall_model.place(ids, offsets, fixed, op_or, keep)
            op = model.OR if op_or else model.ANDNOT
            assert np.array_equal(model.place_affine(ids, maps, None, fixed, op, keep), want)
            assert np.array_equal(model.place_affine(ids, maps, model.moved_boxes(rec, offsets, S), fixed, op, keep), want)


def test_model_cases_are_what_they_claim():
    """the combs put exactly two ids into every word between the planes; the checkerboard is one-voxel pieces; the pose case
    has pieces that touch, pieces that overlap in dst, skipped boxes and a dropped piece"""
    S = 16
    ids, rec = components_model.label(model.combs(S), 6)
    assert len(rec) == 2
    for x in range(2, S - 2, 2):
        for y in range(0, S, 2):
            for z in range(0, S, 8):
                word = ids[x:x + 2, y:y + 2, z:z + 8]
                assert set(np.unique(word).tolist()) == {0, 1, int(NONE)}
    ids, rec = components_model.label(model.checkerboard(S), 6)
    assert len(rec) == S ** 3 // 2 == 2048 and (rec["voxels"] == 1).all()
    debris, ids, maps, boxes, keep, base = model.pose_case(32, 5)
    assert len(maps) > 40 and 0 < keep.sum() < len(keep)
    assert len(components_model.label(debris, 26)[1]) < len(maps)            # pieces touch by edges or corners
    each = [model.place_affine(ids, [mp if j == i else (mp[0], [1 << 50] * 3) for j, mp in enumerate(maps)], boxes, np.zeros_like(base)) for i in range(len(maps))]
    assert (np.sum(each, axis=0) > 1).any()                                  # two pieces land on the same voxel


# ---- vrc_affine_place_box ------------------------------------------------------------------------------------------

def rotations():
    r = stamp_model.rotation
    return [r(0, 0.0), r(2, np.pi / 2), stamp_model.compose(r(0, np.pi / 6), r(1, np.pi / 6)), stamp_model.compose(r(1, 1.1), r(2, -2.3)), r(1, 0.3)]


def test_place_box_with_the_full_cube_is_affine_place(built):
    import cpuvoxelraycaster_amd as vrc
    for depth in range(2, 11):
        S = 1 << depth
        for rot in rotations():
            for scale in (1.0, 0.5, 2.0, 0.3):
                sp, dp = (S / 2, S / 3, S / 2 + 0.25), (S / 2 + 1.5, S / 2, S / 4)
                a, lo, hi = vrc.affine_place(rot, scale, sp, dp, depth, depth)
                b, blo, bhi = vrc.affine_place_box(rot, scale, sp, dp, (0, 0, 0), (S, S, S), depth)
                assert bytes(a) == bytes(b) and lo == blo and hi == bhi, (depth, scale)


def test_place_box_on_sub_boxes_is_the_model(built):
    import cpuvoxelraycaster_amd as vrc
    rng = np.random.default_rng(11)
    empty = 0
    for depth in (3, 5, 9):
        S = 1 << depth
        for rot in rotations():
            for scale in (1.0, 0.7, 3.0):
                slo = rng.integers(0, S, 3)
                shi = slo + rng.integers(0, S // 2, 3)
                sp = (slo + shi) / 2 + rng.uniform(-1, 1, 3)
                dp = rng.uniform(-S / 4, S + S / 4, 3)
                a, lo, hi = vrc.affine_place_box(rot, scale, sp, dp, slo, shi, depth)
                m, t, mlo, mhi = model.place_box(rot, scale, sp, dp, slo, shi, depth)
                assert (list(a.m), list(a.t), a.reserved) == (m, t, 0) and (list(lo), list(hi)) == (mlo, mhi)
                empty += hi == (0, 0, 0)
    assert empty                                                             # a box that leaves dst altogether occurred


def test_place_box_refusals(built):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    rot, sp, dp = stamp_model.rotation(0, 0.4), np.ones(3, np.float32), np.ones(3, np.float32)
    slo, shi = np.zeros(3, np.uint32), np.full(3, 8, np.uint32)
    a, lo, hi = capi.Affine(), np.full(3, 7, np.uint32), np.full(3, 7, np.uint32)
    a.reserved = 55
    good = [capi.ptr(rot), 1.0, capi.ptr(sp), capi.ptr(dp), capi.ptr(slo), capi.ptr(shi), 5, C.byref(a), capi.ptr(lo), capi.ptr(hi)]

    def refused(text, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        assert L.vrc_affine_place_box(*args) == -1
        assert L.vrc_last_error().startswith(b"vrc_affine_place_box: " + text), L.vrc_last_error()
        assert a.reserved == 55 and (lo == 7).all() and (hi == 7).all()
    for i in (0, 2, 3, 4, 5, 7, 8, 9):
        refused(b"null argument", **{"a%d" % i: None})
    refused(b"depth 1 not in [2,10]", a6=1)
    refused(b"depth 11 not in [2,10]", a6=11)
    refused(b"NaN or infinite input", a1=float("nan"))
    bad = rot.copy()
    bad[4] = np.nan
    refused(b"NaN or infinite input", a0=capi.ptr(bad))
    bad = sp.copy()
    bad[2] = np.inf
    refused(b"NaN or infinite input", a2=capi.ptr(bad))
    refused(b"NaN or infinite input", a3=capi.ptr(bad))
    refused(b"scale 0 is not positive", a1=0.0)
    refused(b"scale 0.05 below 1/16", a1=0.05)
    refused(b"source box inverted on axis 1: 9 above 8", a4=capi.ptr(np.array([0, 9, 0], np.uint32)))
    refused(b"t[0] = ", a2=capi.ptr(np.full(3, 1e9, np.float32)))
    assert L.vrc_affine_place_box(*good) == 0 and a.reserved == 0


# ---- refusals of the device calls ----------------------------------------------------------------------------------

def affine(m=None, t=None, reserved=0):
    from cpuvoxelraycaster_amd import capi
    a = np.zeros(1, capi.AFFINE_DTYPE)
    a["m"][0] = [65536, 0, 0, 0, 65536, 0, 0, 0, 65536] if m is None else m
    a["t"][0] = [0, 0, 0] if t is None else t
    a["reserved"][0] = reserved
    return a


def test_rigid_refusals_need_no_gpu(built):
    """NULLs, REPLACE, a bad mem kind, an unknown op, a device mismatch, maps beyond the limits and reserved != 0 are
    VRC_ERR_INVALID with the function's name before any HIP call: the handles here are not volumes or labels at all, and
    nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b, c, one = (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)()
    for i in range(128):
        c[i] = 0x01010101                                                     # every field differs, and as labels C > 0
    one[2] = 1                                                                # labels: device 0, depth 0, count 1 (uint64 at byte 8)
    pa, pb, pc, p1 = (C.cast(v, C.c_void_p) for v in (a, b, c, one))
    out = np.full(3, 9, capi.MOMENTS_DTYPE)
    good = affine()
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_rigid_moments(None, 0, 3, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_moments: null labels"
        assert L.vrc_rigid_moments(pa, 0, 3, None, mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_moments: null buffer with capacity 3"
        assert L.vrc_rigid_place_affine(None, None, capi.ptr(good), None, pb, capi.VRC_COPY_OR, mem, None) == -1
        assert L.vrc_rigid_place_affine(pa, None, capi.ptr(good), None, None, capi.VRC_COPY_OR, mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_place_affine: null argument"
        for op in (-1, 3, 26):
            assert L.vrc_rigid_place_affine(pa, None, capi.ptr(good), None, pb, op, mem, None) == -1
            assert L.vrc_last_error() == b"vrc_rigid_place_affine: bad op %d" % op
        assert L.vrc_rigid_place_affine(pa, None, capi.ptr(good), None, pb, capi.VRC_COPY_REPLACE, mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_rigid_place_affine: VRC_COPY_REPLACE"), L.vrc_last_error()
        for op in (capi.VRC_COPY_OR, capi.VRC_COPY_ANDNOT):
            assert L.vrc_rigid_place_affine(pa, None, capi.ptr(good), None, pc, op, mem, None) == -1
            assert L.vrc_last_error() == b"vrc_rigid_place_affine: labels on device 0, volume on device 16843009"
            assert L.vrc_rigid_place_affine(p1, None, None, None, pb, op, mem, None) == -1
            assert L.vrc_last_error() == b"vrc_rigid_place_affine: null maps with 1 components"
    for mem in (-1, 2, 7):
        assert L.vrc_rigid_moments(pa, 0, 3, capi.ptr(out), mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_moments: bad mem kind %d" % mem
        assert L.vrc_rigid_place_affine(pa, None, capi.ptr(good), None, pb, capi.VRC_COPY_OR, mem, None) == -1
        assert L.vrc_last_error() == b"vrc_rigid_place_affine: bad mem kind %d" % mem
    # host memory: the maps are read and checked before any device call
    limit_m, limit_t = 1 << 20, 1 << 40
    for bad, text in ((affine(reserved=1), b"piece 0: reserved is 1, not 0"),
                      (affine(m=[limit_m + 1] + [0] * 8), b"piece 0: m[0] = 1048577 beyond +-2^20"),
                      (affine(m=[0] * 8 + [-limit_m - 1]), b"piece 0: m[8] = -1048577 beyond +-2^20"),
                      (affine(t=[limit_t + 1, 0, 0]), b"piece 0: t[0] = 1099511627777 beyond +-2^40"),
                      (affine(t=[0, 0, -limit_t - 1]), b"piece 0: t[2] = -1099511627777 beyond +-2^40")):
        for op in (capi.VRC_COPY_OR, capi.VRC_COPY_ANDNOT):
            assert L.vrc_rigid_place_affine(p1, None, capi.ptr(bad), None, pb, op, capi.VRC_MEM_HOST, None) == -1
            assert L.vrc_last_error() == b"vrc_rigid_place_affine: " + text, L.vrc_last_error()
    # no pieces, an empty window: legal without a device, nothing written
    assert L.vrc_rigid_moments(pa, 0, 3, capi.ptr(out), capi.VRC_MEM_HOST, None) == 0
    assert L.vrc_rigid_moments(p1, 1, 3, capi.ptr(out), capi.VRC_MEM_DEVICE, None) == 0          # first >= C
    assert L.vrc_rigid_moments(p1, 0, 0, None, capi.VRC_MEM_HOST, None) == 0                     # capacity 0, no buffer
    assert L.vrc_rigid_place_affine(pa, None, None, None, pb, capi.VRC_COPY_ANDNOT, capi.VRC_MEM_HOST, None) == 0
    assert out.tobytes() == np.full(3, 9, capi.MOMENTS_DTYPE).tobytes()
    assert not any(a) and not any(b) and all(v == 0x01010101 for v in c) and list(one) == [0, 0, 1] + [0] * 125


def test_struct_sizes(built):
    from cpuvoxelraycaster_amd import capi
    assert capi.MOMENTS_DTYPE.itemsize == 80 and capi.AFFINE_DTYPE.itemsize == 64 and C.sizeof(capi.Affine) == 64
    assert [capi.MOMENTS_DTYPE.fields[f][1] for f in ("voxels", "s1", "s2")] == [0, 8, 32]
    assert [capi.AFFINE_DTYPE.fields[f][1] for f in ("m", "reserved", "t")] == [capi.Affine.m.offset, capi.Affine.reserved.offset, capi.Affine.t.offset] == [0, 36, 40]
    src = ('#include "%s"\n#include <stddef.h>\n'
           'static_assert(sizeof(vrc_piece_moments) == 80 && offsetof(vrc_piece_moments, s1) == 8 && offsetof(vrc_piece_moments, s2) == 32, "moments");\n'
           'static_assert(sizeof(vrc_affine) == 64, "affine");\n') % os.path.join(ROOT, "include", "vrc.h")
    check_cpp_syntax(src)


# ---- mass properties -----------------------------------------------------------------------------------------------

def test_mass_properties_round_the_exact_value_once(built):
    """fixed integer sums, large ones included (a 1024^3 solid: sums near 2^52, where float64 arithmetic on the raw sums
    would lose the low bits): every entry equals float(Fraction)"""
    import cpuvoxelraycaster_amd as vrc
    ids = np.full((8, 8, 8), NONE, np.uint32)
    ids[1:4, 2:7, 0:3] = 0
    ids[5, 5, 5] = ids[6, 5, 5] = ids[6, 6, 5] = ids[6, 6, 6] = 1
    ids[7, 0, 1] = 2
    cases = model.moments(ids) + [model.solid_cube_moments(1024), model.solid_cube_moments(128)]
    n, s1, s2 = model.solid_cube_moments(1024)
    cases.append((n - 1, [v - 2047 for v in s1], [v - 2047 * 2047 for v in s2]))       # the same without its last voxel
    rec = np.zeros(len(cases) + 1, vrc.capi.MOMENTS_DTYPE)                             # and an empty record at the end
    for i, (n, s1, s2) in enumerate(cases):
        rec[i] = (n, s1, s2)
    mass, centre, inertia = vrc.mass_properties(rec)
    assert mass.dtype == centre.dtype == inertia.dtype == np.float64
    assert centre.shape == (len(rec), 3) and inertia.shape == (len(rec), 3, 3)
    for i, case in enumerate(cases):
        m, c, I = model.mass_properties(*case)
        assert mass[i] == float(m)
        assert centre[i].tolist() == [float(v) for v in c]
        assert inertia[i].tolist() == [[float(v) for v in row] for row in I], i
    assert mass[-1] == 0 and not centre[-1].any() and not inertia[-1].any()
    assert inertia[2].tolist() == [[1 / 6, 0, 0], [0, 1 / 6, 0], [0, 0, 1 / 6]]


def test_python_arguments(built):
    import cpuvoxelraycaster_amd as vrc
    labels = vrc.VoxelLabels(None, 2, 4, 0)
    two = np.zeros(2, vrc.capi.AFFINE_DTYPE)
    with pytest.raises(ValueError, match="maps"):
        labels.placeAffine(np.zeros(3, vrc.capi.AFFINE_DTYPE))
    with pytest.raises(ValueError, match="boxes"):
        labels.placeAffine(two, boxes=np.zeros((1, 6), np.uint32))
    with pytest.raises(ValueError, match="keep"):
        labels.placeAffine(two, keep=[1])
    a = vrc.make_affine(range(9), [5, -6, 1 << 39])
    arr = vrc.raycaster.affine_array([a, a])
    assert arr.tobytes() == bytes(a) * 2


def test_host_adapter_with_rigid_compiles(built):
    """HipVoxelLabels::moments / poses / placeAffine in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& debris) {\n'
           '    vrc_host::HipVoxelLabels labels = debris.labelComponents(6, false);\n'
           '    std::vector<vrc_piece_moments> mo = labels.moments();\n'
           '    std::vector<vrc_host::HipMassProperties> mp = labels.massProperties();\n'
           '    std::vector<float> rot(9, 0.0f), pivots(3 * labels.count(), 1.0f);\n'
           '    std::vector<uint32_t> boxes;\n'
           '    std::vector<vrc_affine> maps = labels.poses(rot.data(), pivots, world.depth(), boxes);\n'
           '    labels.placeAffine(maps, world, VRC_COPY_OR, &boxes);\n'
           '    std::vector<uint8_t> keep(labels.count(), 1);\n'
           '    labels.placeAffine(maps, world, VRC_COPY_ANDNOT, nullptr, &keep);\n'
           '    return mo.size() + (uint64_t)mp[0].mass + labels.moments(1, 2).size();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
