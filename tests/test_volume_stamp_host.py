"""The affine stamp on a machine without a GPU: the yardstick of the GPU tests itself -- the numpy model of
tests/stamp_model.py against the definition taken literally (a triple loop in Python's unbounded integers) and against
np.transpose / np.flip on the 48 signed permutations --, the map record's size, the refusals that need no device,
vrc_affine_place by its properties, and the C++ host adapter's new members under a plain C++14 compiler."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import stamp_model as model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def literal_stamp(dst, src, m, t, lo, hi, op):
    """include/vrc.h word for word, voxel by voxel, in Python ints"""
    Sd, Ss = dst.shape[0], src.shape[0]
    out = dst.copy()
    for x in range(max(lo[0], 0), min(hi[0], Sd)):
        for y in range(max(lo[1], 0), min(hi[1], Sd)):
            for z in range(max(lo[2], 0), min(hi[2], Sd)):
                c = (2 * x + 1, 2 * y + 1, 2 * z + 1)
                q = []
                for a in range(3):
                    s = int(m[3 * a]) * c[0] + int(m[3 * a + 1]) * c[1] + int(m[3 * a + 2]) * c[2] + int(t[a])
                    assert abs(s) < 1 << 41
                    q.append(s >> 17)                     # Python's shift of a negative int is floor as well
                bit = int(src[q[0], q[1], q[2]]) if all(0 <= v < Ss for v in q) else 0
                if op == model.REPLACE:
                    out[x, y, z] = bit
                elif op == model.OR:
                    out[x, y, z] |= bit
                else:
                    out[x, y, z] &= 1 - bit
    return out


def random_maps(rng, Ss, Sd, count):
    """maps up to the limits, and maps aimed at the source so that the stamp is not empty"""
    maps = []
    aimed = model.aimed_maps(rng, Ss, Sd, count)
    for i in range(count):
        if i % 3 == 0:
            m = rng.integers(-model.M_LIMIT, model.M_LIMIT + 1, 9)
            t = rng.integers(-model.T_LIMIT, model.T_LIMIT + 1, 3)
        elif i % 3 == 1:
            m = rng.integers(-model.M_LIMIT, model.M_LIMIT + 1, 9)
            t = rng.integers(-(Ss << 21), (Ss << 21) + 1, 3)
        else:
            m, t = aimed[i]
        maps.append(([int(v) for v in m], [int(v) for v in t]))
    limit = [model.M_LIMIT, -model.M_LIMIT] * 4 + [model.M_LIMIT]
    maps.append((limit, [model.T_LIMIT, -model.T_LIMIT, model.T_LIMIT]))
    maps.append(([-v for v in limit], [-model.T_LIMIT, model.T_LIMIT, -model.T_LIMIT]))
    return maps


@pytest.mark.parametrize("Sd,Ss", [(4, 8), (8, 4), (8, 16)])
def test_model_against_the_definition(Sd, Ss):
    rng = np.random.default_rng(4100 + Sd + Ss)
    src = (rng.random((Ss, Ss, Ss)) < 0.4).astype(np.uint8)
    dst = (rng.random((Sd, Sd, Sd)) < 0.5).astype(np.uint8)
    boxes = [((0, 0, 0), (Sd, Sd, Sd)), ((1, 0, 1), (Sd - 1, Sd, Sd + 5)), ((1, 2, 3), (2, 3, 4)), ((2, 2, 2), (2, 5, 5)), ((3, 1, 0), (1, 4, 4))]
    hit = 0
    for i, (m, t) in enumerate(random_maps(rng, Ss, Sd, 24)):
        lo, hi = boxes[i % len(boxes)]
        for op in (model.REPLACE, model.OR, model.ANDNOT):
            got = model.stamp(dst, src, m, t, lo, hi, op)
            assert got.dtype == np.uint8 and np.array_equal(got, literal_stamp(dst, src, m, t, lo, hi, op)), (m, t, lo, hi, op)
        hit += int(model.stamp(np.zeros_like(dst), src, m, t).any())
    assert hit >= 6                                       # the aimed maps do read the source
    # the defaults: the whole volume, REPLACE
    m, t = model.IDENTITY
    assert np.array_equal(model.stamp(dst, src, m, t), literal_stamp(dst, src, m, t, (0, 0, 0), (Sd, Sd, Sd), model.REPLACE))


def test_model_on_the_48_signed_permutations():
    S = 8
    rng = np.random.default_rng(48)
    src = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
    empty = np.zeros_like(src)
    cases = model.all_signed_permutations()
    assert len(cases) == 48
    images = set()
    for perm, flip in cases:
        m, t = model.signed_permutation(perm, flip, S)
        got = model.stamp(empty, src, m, t)
        assert np.array_equal(got, model.permuted(src, perm, flip)), (perm, flip)
        assert int(got.sum()) == int(src.sum())           # a bijection
        images.add(got.tobytes())
    assert len(images) == 48
    # the header's example: q = (p_y, S-1-p_x, p_z)
    m, t = model.signed_permutation((1, 0, 2), (0, 1, 0), S)
    assert m == [0, 65536, 0, -65536, 0, 0, 0, 0, 65536] and t == [0, S << 17, 0]
    turned = model.stamp(empty, src, m, t)
    p = np.indices((S, S, S))
    assert np.array_equal(turned, src[p[1], S - 1 - p[0], p[2]])
    # identity, halving by point sampling and doubling by replication
    assert np.array_equal(model.stamp(empty, src, *model.IDENTITY), src)
    half = model.stamp(np.zeros((4, 4, 4), np.uint8), src, [2 * 65536, 0, 0, 0, 2 * 65536, 0, 0, 0, 2 * 65536], [0, 0, 0])
    assert np.array_equal(half, src[1::2, 1::2, 1::2])    # the centre 2p + 1 of the coarse voxel lies in fine voxel 2p + 1
    twice = model.stamp(np.zeros((16, 16, 16), np.uint8), src, [32768, 0, 0, 0, 32768, 0, 0, 0, 32768], [0, 0, 0])
    assert np.array_equal(twice, src.repeat(2, 0).repeat(2, 1).repeat(2, 2))


def test_python_permutation_helper_is_the_models(built):
    import cpuvoxelraycaster_amd as vrc
    for perm, flip in model.all_signed_permutations():
        for size in (4, 8, 1024):
            a = vrc.affine_signed_permutation(perm, flip, size)
            assert (list(a.m), list(a.t), a.reserved) == (*model.signed_permutation(perm, flip, size), 0)
    a = vrc.make_affine([-(1 << 20)] * 9, [1 << 40, -(1 << 40), 5])
    assert list(a.m) == [-(1 << 20)] * 9 and list(a.t) == [1 << 40, -(1 << 40), 5]


def test_affine_layout(built):
    from cpuvoxelraycaster_amd import capi
    assert C.sizeof(capi.Affine) == 64 and capi.VRC_AFFINE_FRAC_BITS == 16
    assert [getattr(capi.Affine, f).offset for f in ("m", "reserved", "t")] == [0, 36, 40]
    hdr = os.path.join(ROOT, "include", "vrc.h")
    src = ('#include "%s"\nstatic_assert(sizeof(vrc_affine) == 64, "vrc_affine");\n'
           'static_assert(VRC_AFFINE_FRAC_BITS == 16, "VRC_AFFINE_FRAC_BITS");\nint main() { return 0; }\n') % hdr
    check_cpp_syntax(src)


def test_stamp_refusals_need_no_gpu(built):
    """NULL arguments, src == dst, an unknown op, reserved != 0, an |m| entry above 2^20, a |t| entry above 2^40 and volumes
    on different devices are VRC_ERR_INVALID with the function's name before any HIP call: the handles here are not volumes
    at all, and nothing is written."""
    import cpuvoxelraycaster_amd as vrc
    capi = vrc.capi
    L = capi.load()
    a, b = (C.c_uint32 * 128)(), (C.c_uint32 * 128)()        # 512 zero bytes each: "depth 0 on device 0" whatever the layout
    pa, pb = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    lo, hi = np.zeros(3, np.uint32), np.full(3, 4, np.uint32)
    good = vrc.make_affine(*model.IDENTITY)
    name = b"vrc_volume_stamp_affine"

    def refused(dst, src, amap, lo_, hi_, op, text=b""):
        assert L.vrc_volume_stamp_affine(dst, src, amap, lo_, hi_, op, None) == -1
        err = L.vrc_last_error()
        assert err.startswith(name) and text in err, err

    for args in [(None, pb), (pa, None)]:
        refused(*args, C.byref(good), capi.ptr(lo), capi.ptr(hi), 0, b"null")
    refused(pa, pb, None, capi.ptr(lo), capi.ptr(hi), 0, b"null")
    refused(pa, pb, C.byref(good), None, capi.ptr(hi), 0, b"null")
    refused(pa, pb, C.byref(good), capi.ptr(lo), None, 0, b"null")
    refused(pa, pa, C.byref(good), capi.ptr(lo), capi.ptr(hi), 0, b"same volume")
    for op in (-1, 3, 26):
        refused(pa, pb, C.byref(good), capi.ptr(lo), capi.ptr(hi), op, b"bad op")
    bad = vrc.make_affine(*model.IDENTITY)
    bad.reserved = 1
    refused(pa, pb, C.byref(bad), capi.ptr(lo), capi.ptr(hi), 1, b"reserved")
    for i in range(9):
        for v in ((1 << 20) + 1, -(1 << 20) - 1, 0x7FFFFFFF, -0x80000000):
            m = list(model.IDENTITY[0])
            m[i] = v
            refused(pa, pb, C.byref(vrc.make_affine(m, [0, 0, 0])), capi.ptr(lo), capi.ptr(hi), 2, b"m[%d]" % i)
    for i in range(3):
        for v in ((1 << 40) + 1, -(1 << 40) - 1, (1 << 63) - 1, -(1 << 63)):
            t = [0, 0, 0]
            t[i] = v
            refused(pa, pb, C.byref(vrc.make_affine(model.IDENTITY[0], t)), capi.ptr(lo), capi.ptr(hi), 0, b"t[%d]" % i)
    # a volume whose every field differs from the other's: a device mismatch
    for i in range(128):
        b[i] = 0x01010101
    at_limit = vrc.make_affine([1 << 20, -(1 << 20)] * 4 + [1 << 20], [1 << 40, -(1 << 40), 1 << 40])
    for amap in (good, at_limit):
        for op in (0, 1, 2):
            refused(pa, pb, C.byref(amap), capi.ptr(lo), capi.ptr(hi), op, b"devices")
    assert not any(a) and all(v == 0x01010101 for v in b)
    assert list(lo) == [0, 0, 0] and list(hi) == [4, 4, 4]
    # the Python class hands the refusal on
    fake = vrc.VoxelVolume.__new__(vrc.VoxelVolume)
    fake._h, fake.depth, fake.device = None, 3, 0
    with pytest.raises(vrc.VrcError, match="vrc_volume_stamp_affine"):
        fake.stampAffine(fake, good)


def test_affine_place_refusals(built):
    import cpuvoxelraycaster_amd as vrc
    capi = vrc.capi
    L = capi.load()
    rot = np.eye(3, dtype=np.float32).reshape(9)
    sp, dp = np.full(3, 8, np.float32), np.full(3, 16, np.float32)
    lo, hi = np.full(3, 7, np.uint32), np.full(3, 7, np.uint32)
    out = capi.Affine()
    out.reserved = 9

    def call(rot_=rot, scale=1.0, sp_=sp, dp_=dp, sd=4, dd=5, out_=C.byref(out), lo_=lo, hi_=hi):
        return L.vrc_affine_place(capi.ptr(rot_), scale, capi.ptr(sp_), capi.ptr(dp_), sd, dd, out_, capi.ptr(lo_), capi.ptr(hi_))

    refusals = [dict(rot_=None), dict(sp_=None), dict(dp_=None), dict(out_=None), dict(lo_=None), dict(hi_=None),
                dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
                dict(scale=0.0624), dict(scale=1e-30),
                dict(sd=1), dict(sd=11), dict(dd=1), dict(dd=11), dict(sd=0), dict(dd=0xFFFFFFFF)]
    for bad in (float("nan"), float("inf"), -float("inf")):
        for i in range(9):
            r = rot.copy()
            r[i] = bad
            refusals.append(dict(rot_=r))
        for i in range(3):
            p = sp.copy()
            p[i] = bad
            refusals += [dict(sp_=p), dict(dp_=p)]
    refusals.append(dict(rot_=(rot * 2).astype(np.float32), scale=0.0625))          # m = 2^21
    refusals.append(dict(sp_=np.full(3, 2.0 ** 24, np.float32)))                     # t = 2^41
    for kw in refusals:
        assert call(**kw) == -1, kw
        assert L.vrc_last_error().startswith(b"vrc_affine_place"), L.vrc_last_error()
    assert out.reserved == 9 and (lo == 7).all() and (hi == 7).all()                  # a refusal writes nothing
    # the limit itself is legal: scale 1/16 gives m = 2^20
    assert call(scale=0.0625) == 0
    assert list(out.m) == [1 << 20, 0, 0, 0, 1 << 20, 0, 0, 0, 1 << 20] and out.reserved == 0
    with pytest.raises(vrc.VrcError, match="vrc_affine_place"):
        vrc.affine_place(rot, 0.01, sp, dp, 4, 5)


def placements():
    """a dozen rotations x scales from 0.25 to 4, pivots on and off the lattice"""
    quarter = np.pi / 2
    rots = [np.eye(3, dtype=np.float32).reshape(9), model.rotation(2, quarter), model.rotation(0, np.pi), model.rotation(1, 0.3),
            model.rotation(2, np.radians(30)), model.rotation(0, np.radians(45)), model.rotation(1, -1.1),
            model.compose(model.rotation(0, np.radians(30)), model.rotation(1, np.radians(30))),
            model.compose(model.rotation(2, 2.0), model.rotation(0, -0.7)),
            model.compose(model.rotation(1, 0.9), model.compose(model.rotation(2, 0.4), model.rotation(0, 2.5))),
            model.compose(model.rotation(0, np.radians(45)), model.rotation(1, np.arctan(1 / np.sqrt(2)))),
            model.compose(model.rotation(2, -3.0), model.rotation(1, 1.3))]
    scales = [0.25, 0.5, 0.8, 1.0, 1.5, 2.0, 3.0, 4.0]
    pivots = [((8.0, 8.0, 8.0), (16.0, 16.0, 16.0)), ((0.0, 0.0, 0.0), (10.5, 3.25, 20.0)), ((8.5, 3.0, 16.0), (31.0, 0.0, 15.5)),
              ((8.0, 8.0, 8.0), (-20.0, 16.0, 16.0)), ((8.0, 8.0, 8.0), (200.0, 200.0, 200.0))]
    cases = []
    for i, rot in enumerate(rots):
        for j, scale in enumerate(scales):
            cases.append((rot, scale, *pivots[(i + j) % len(pivots)]))
    return cases


def test_affine_place_by_properties(built):
    import cpuvoxelraycaster_amd as vrc
    sd, dd = 4, 5
    Ss, Sd = 1 << sd, 1 << dd
    full = np.ones((Ss, Ss, Ss), np.uint8)
    empty = np.zeros((Sd, Sd, Sd), np.uint8)
    seen_empty = seen_clipped = 0
    for rot, scale, sp, dp in placements():
        a, lo, hi = vrc.affine_place(rot, scale, sp, dp, sd, dd)
        m, t = list(a.m), list(a.t)
        assert a.reserved == 0
        # every entry within half a unit of 65536 R^T / scale; in rot's column layout R^T[a][b] is rot[3a + b]
        ideal = 65536.0 * np.asarray(rot, np.float64) / float(np.float32(scale))
        assert np.abs(np.asarray(m, np.float64) - ideal).max() <= 0.5 + 1e-6, (scale, m)
        # t within 1 of the exact rational value for the RETURNED m: the pivot maps to the pivot
        for ax in range(3):
            exact = 131072 * Fraction(float(np.float32(sp[ax]))) - sum(2 * m[3 * ax + b] * Fraction(float(np.float32(dp[b]))) for b in range(3))
            assert abs(t[ax] - exact) <= 1, (scale, ax, t[ax], float(exact))
        # the Python mirror of the formulas gives the same record and box
        assert (m, t, list(lo), list(hi)) == tuple(model.place(rot, scale, sp, dp, sd, dd))
        # the box: inside the destination, and no destination voxel outside it maps into the source
        assert all(0 <= l <= h <= Sd for l, h in zip(lo, hi))
        reads = model.stamp(empty, full, m, t)
        outside = reads.copy()
        outside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 0
        assert not outside.any(), (scale, sp, dp, lo, hi)
        if not reads.any():
            seen_empty += 1
        if lo == hi == (0, 0, 0):
            assert not reads.any()
        elif any(l > 0 for l in lo) or any(h < Sd for h in hi):
            seen_clipped += 1
    assert seen_empty >= 8 and seen_clipped >= 20


def test_host_adapter_with_stamp_compiles(built):
    """HipVoxelVolume::stampAffine / stampPlaced in the header-only adapter: C++14, no GLM, no HIP headers; and the GPU
    test's program."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'vrc_affine use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& clipboard) {\n'
           '    vrc_affine turn = {{0, 65536, 0, -65536, 0, 0, 0, 0, 65536}, 0, {0, (int64_t)64 << 17, 0}};\n'
           '    world.stampAffine(clipboard, turn);\n'
           '    const uint32_t lo[3] = {1, 2, 3}, hi[3] = {30, 31, 32};\n'
           '    world.stampAffine(clipboard, turn, lo, hi, VRC_COPY_ANDNOT, nullptr);\n'
           '    float rot[9];\n'
           '    vrc_make_rotation(0.5f, 0.25f, rot);\n'
           '    const float pivot[3] = {1.5f, 2.0f, 3.0f};\n'
           '    world.stampPlaced(clipboard, rot);\n'
           '    return world.stampPlaced(clipboard, rot, 1.5f, pivot, pivot, VRC_COPY_REPLACE, nullptr);\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
    main = os.path.join(ROOT, "tests", "cpp", "voxel_stamp_main.cpp")
    check_cpp_syntax(main, strict=True)
