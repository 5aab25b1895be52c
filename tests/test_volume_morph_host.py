"""vrc_morph_apply without a GPU: the numpy model (morph_model.py) against the rule of include/vrc.h taken literally in Python
loops, the duality and the composition of Minkowski sums in the model, element_ball against the distance model, every refusal
that precedes a device call by its whole text, the symbols, and the C++ adapter's new methods."""
import ctypes as C
import os

import numpy as np
import pytest

import distance_model
import morph_model as model
from volume_support import ROOT, check_cpp_syntax


def literal(vol, what, offsets, of, outside, origin=(0, 0, 0)):
    """the header's rule voxel by voxel, as nested lists"""
    S = len(vol)
    E = {(o[0] - origin[0], o[1] - origin[1], o[2] - origin[2]) for o in offsets}

    def in_a(q):
        if min(q) < 0 or max(q) >= S:
            return outside != 0
        solid = vol[q[0]][q[1]][q[2]] != 0
        return solid if of == model.SOLID else not solid

    out = [[[0] * S for _ in range(S)] for _ in range(S)]
    for x in range(S):
        for y in range(S):
            for z in range(S):
                if what == model.DILATE:
                    out[x][y][z] = int(any(in_a((x - e[0], y - e[1], z - e[2])) for e in E))
                else:
                    out[x][y][z] = int(all(in_a((x + e[0], y + e[1], z + e[2])) for e in E))
    return out


def elements(S, rng):
    return [model.cross(), model.box(2, 3, 1, (0, 2, 0)), model.line(2, -S, S - 1), model.ball(2), np.zeros((0, 3), np.int32),
            np.array([(0, 0, 0)], np.int32), np.array([(16, -16, 5), (-3, 0, 1)], np.int32), model.random_element(rng, 12, S),
            np.repeat(model.random_element(rng, 5, 3), 3, axis=0)]


@pytest.mark.parametrize("S", [4, 8])
def test_model_is_the_header(S):
    rng = np.random.default_rng(70 + S)
    vol = model.source(S)
    for e in elements(S, rng):
        for what in (model.DILATE, model.ERODE):
            for of in (model.SOLID, model.EMPTY):
                for outside in (0, 1):
                    got = model.morph(vol, what, e, of, outside)
                    assert got.dtype == np.uint8 and got.tolist() == literal(vol.tolist(), what, e.tolist(), of, outside), (S, e.tolist(), what, of, outside)
    # the origin is subtracted, and a uint32 list is an int32 list
    e = np.array([(5, 6, 7), (6, 6, 7), (5, 4, 7)], np.uint32)
    assert model.morph(vol, model.DILATE, e, origin=(5, 5, 7)).tolist() == literal(vol.tolist(), model.DILATE, e.tolist(), model.SOLID, 0, (5, 5, 7))
    # n == 0, the formulas taken literally
    assert model.morph(vol, model.DILATE, []).sum() == 0 and model.morph(vol, model.ERODE, []).sum() == S ** 3


@pytest.mark.parametrize("S", [8, 16])
def test_model_duality_and_composition(S):
    rng = np.random.default_rng(S)
    vol = model.source(S)
    for e in [model.cross(), model.box(3, 2, 4, (2, 0, 1)), model.random_element(rng, 20, 5), np.zeros((0, 3), np.int32)]:
        for of, other in ((model.SOLID, model.EMPTY), (model.EMPTY, model.SOLID)):
            for outside in (0, 1):
                eroded = model.morph(vol, model.ERODE, e, of, outside)
                assert np.array_equal(eroded, 1 - model.morph(vol, model.DILATE, model.reflect(e), other, 1 - outside))
    # A box is three lines in a row.  Clipping between the steps loses nothing: a line moves one coordinate, so a voxel that
    # an intermediate volume clips has that coordinate outside in every voxel it would have led to.
    for (a, b, c), anchor in [((3, 5, 3), (1, 2, 1)), ((4, 2, 9), (0, 1, 8))]:
        for outside in (0, 1):
            step = vol
            for axis, (length, at) in enumerate(zip((a, b, c), anchor)):
                step = model.morph(step, model.DILATE, model.line(axis, -at, length - 1 - at), outside=outside)
            assert np.array_equal(step, model.morph(vol, model.DILATE, model.box(a, b, c, anchor), outside=outside))
    # fits_at by hand: a 3 x 5 x 3 room has one pivot for its own box and none for a larger one
    room = np.ones((8, 8, 8), np.uint8)
    room[2:5, 1:6, 3:6] = 0
    assert np.argwhere(model.fits_at(room, model.box(3, 5, 3))).tolist() == [[3, 3, 4]]
    assert model.fits_at(room, model.box(3, 5, 4)).sum() == 0 and model.fits_at(room, model.box(2, 5, 3)).sum() == 2
    # match against its definition
    solid_at, empty_at = [(0, 0, 0), (0, -1, 0)], [(1, 0, 0), (0, 0, 1), (0, 0, 2)]
    for outside in (0, 1):
        def solid(q):
            return bool(vol[q]) if min(q) >= 0 and max(q) < S else bool(outside)
        want = [list(q) for q in np.ndindex(S, S, S)
                if all(solid((q[0] + s[0], q[1] + s[1], q[2] + s[2])) for s in solid_at) and not any(solid((q[0] + t[0], q[1] + t[1], q[2] + t[2])) for t in empty_at)]
        assert np.argwhere(model.match(vol, solid_at, empty_at, outside)).tolist() == want and len(want) > 0


def test_element_helpers():
    import cpuvoxelraycaster_amd as vrc
    vol = model.source(16)
    for r in range(6):
        ball = vrc.element_ball(r)
        assert ball.dtype == np.int32 and sorted(ball.tolist()) == sorted(model.ball(r).tolist())
        assert np.array_equal(model.morph(vol, model.DILATE, ball), distance_model.dilate(vol, r)), r
        for open_border in (False, True):
            assert np.array_equal(model.morph(vol, model.ERODE, ball, outside=int(not open_border)), distance_model.erode(vol, r, open_border)), (r, open_border)
    assert [len(vrc.element_ball(r)) for r in range(4)] == [1, 7, 33, 123]
    for args in [(3, 5, 3), (2, 4, 1), (1, 1, 1)]:
        assert vrc.element_box(*args).tolist() == model.box(*args).tolist()
    assert vrc.element_box(2, 3, 4, (1, 0, 3)).tolist() == model.box(2, 3, 4, (1, 0, 3)).tolist()
    assert vrc.element_box(3, 3, 3).min() == -1 and vrc.element_box(3, 3, 3).max() == 1 and vrc.element_box(4, 4, 4).min() == -2
    assert sorted(vrc.element_cross().tolist()) == sorted(model.cross().tolist())
    for axis in range(3):
        assert vrc.element_line(axis, -16, 16).tolist() == model.line(axis, -16, 16).tolist() and len(vrc.element_line(axis, 0, 0)) == 1
    assert vrc.element_line(1, 2, 1).shape == (0, 3)
    shape = np.zeros((4, 4, 4), np.uint8)
    shape[1, 2, 3] = shape[0, 0, 0] = 1
    assert vrc.element_of(shape, (1, 1, 1)).tolist() == [[-1, -1, -1], [0, 1, 2]]
    assert vrc.reflect([[1, -2, 3]]).tolist() == [[-1, 2, -3]] and vrc.reflect(np.zeros((0, 3))).shape == (0, 3)
    for name in ("element_ball", "element_box", "element_cross", "element_line", "element_of", "reflect"):
        assert name in vrc.__all__
    for name in ("morph", "morphDevice", "dilateBy", "erodeBy", "openBy", "closeBy", "fitsAt", "match"):
        assert callable(getattr(vrc.VoxelVolume, name)), name
    with pytest.raises(ValueError):
        vrc.element_ball(-1)


def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


# `device` is the first 32-bit word of a vrc_volume and `depth` its third
ZERO, OTHER, DEPTH_3, DEVICE_1 = handle(), handle(), handle(w2=3), handle(w0=1)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
GOOD = (C.c_int32 * 6)(16, -16, 0, 1, 2, 3)
FAR = (C.c_int32 * 9)(1, 2, 3, 0, 17, 0, -17, 0, 0)
WIDE = (C.c_int32 * 6)(I32_MAX, 0, 0, 0, 0, I32_MIN)
ORIGIN = (C.c_int32 * 3)(I32_MIN, 1, I32_MAX)
NEAR = (C.c_int32 * 3)(20, 2, -1)


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


def args(dst=ZERO, src=OTHER, what=0, of=1, n=2, offsets=GOOD, origin=None, outside=0, op=0, mem=0):
    return (p(dst), p(src), what, of, n, p(offsets), p(origin), outside, op, mem, None)


# every refusal of vrc_morph_apply that needs no volume, all before the first HIP call: the WHOLE vrc_last_error() text
REFUSALS = [
    (args(dst=None), "null argument"),
    (args(src=None), "null argument"),
    (args(src=ZERO), "source and destination are the same volume"),
    (args(src=DEPTH_3), "volumes of depths 0 and 3"),
    (args(dst=DEVICE_1), "volumes on devices 1 and 0"),
    (args(what=2), "bad what 2"),
    (args(what=-1), "bad what -1"),
    (args(of=0), "bad of 0"),
    (args(of=3), "bad of 3"),
    (args(outside=2), "outside 2 is neither 0 nor 1"),
    (args(outside=-1), "outside -1 is neither 0 nor 1"),
    (args(op=3), "bad op 3"),
    (args(mem=2), "bad mem kind 2"),
    (args(mem=-1), "bad mem kind -1"),
    (args(n=(1 << 20) + 1, mem=1), "1048577 offsets, more than 1048576"),
    (args(n=1 << 63), "9223372036854775808 offsets, more than 1048576"),
    (args(offsets=None), "null offsets"),
    (args(n=1, offsets=None, mem=1), "null offsets"),
    (args(n=3, offsets=FAR), "offset 1 is (0, 17, 0) after the origin, beyond +-16"),
    (args(n=3, offsets=FAR, origin=NEAR), "offset 0 is (-19, 0, 4) after the origin, beyond +-16"),
    (args(n=2, offsets=WIDE, origin=ORIGIN), "offset 0 is (4294967295, -1, -2147483647) after the origin, beyond +-16"),
    (args(n=2, offsets=GOOD, origin=ORIGIN), "offset 0 is (2147483664, -17, -2147483647) after the origin, beyond +-16"),
    # two refusals at once: the one that wins
    (args(src=ZERO, what=2), "source and destination are the same volume"),
    (args(src=DEPTH_3, dst=DEVICE_1), "volumes of depths 0 and 3"),
    (args(src=DEPTH_3, op=3), "volumes of depths 0 and 3"),
    (args(dst=DEVICE_1, of=0), "volumes on devices 1 and 0"),
    (args(src=DEVICE_1, mem=2), "volumes on devices 0 and 1"),
]


def untouched():
    return (not any(ZERO) and not any(OTHER) and list(DEPTH_3) == [0, 0, 3] + [0] * 125 and list(DEVICE_1) == [1] + [0] * 127
            and list(GOOD) == [16, -16, 0, 1, 2, 3] and list(FAR) == [1, 2, 3, 0, 17, 0, -17, 0, 0] and list(ORIGIN) == [I32_MIN, 1, I32_MAX])


@pytest.mark.parametrize("index", range(len(REFUSALS)))
def test_morph_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    call, text = REFUSALS[index]
    assert L.vrc_morph_apply(*call) == -1                                    # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("vrc_morph_apply: %s" % text).encode()
    assert untouched()                                                       # nothing was written through any handle or buffer


def test_symbol_and_constants(built):
    from cpuvoxelraycaster_amd import capi
    assert "vrc_morph_apply" in capi.SYMBOLS and hasattr(C.CDLL(capi.LIB_PATH), "vrc_morph_apply")
    assert (capi.VRC_MORPH_DILATE, capi.VRC_MORPH_ERODE, capi.VRC_MORPH_SOLID, capi.VRC_MORPH_EMPTY) == (model.DILATE, model.ERODE, model.SOLID, model.EMPTY) == (0, 1, 1, 2)
    assert capi.VRC_MORPH_REACH == model.REACH == 16 and capi.VRC_MORPH_MAX_OFFSETS == 1 << 20
    header = open(os.path.join(ROOT, "include", "vrc.h")).read()
    for line in ("#define VRC_MORPH_DILATE 0", "#define VRC_MORPH_ERODE  1", "#define VRC_MORPH_SOLID  1", "#define VRC_MORPH_EMPTY  2", "#define VRC_MORPH_REACH  16",
                 "#define VRC_MORPH_MAX_OFFSETS (1u << 20)"):
        assert line in header, line


def test_host_adapter_with_morph_compiles(built):
    """HipVoxelVolume::morph / morphDevice / dilateBy / erodeBy / openBy / closeBy / fitsAt / match and the element helpers in the
    header-only adapter: C++14, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'size_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& out, const int32_t* list_dev) {\n'
           '    typedef vrc_host::HipVoxelVolume V;\n'
           '    const int32_t anchor[3] = {0, 4, 0}, pivot[3] = {7, 7, 7};\n'
           '    const V::Element ball = V::elementBall(3), box = V::elementBox(3, 5, 3, anchor), line = V::elementLine(0, 0, 6);\n'
           '    world.morph(out, VRC_MORPH_DILATE, ball);\n'
           '    world.morph(out, VRC_MORPH_ERODE, V::elementBox(2, 2, 2), true, true, VRC_COPY_ANDNOT, pivot);\n'
           '    world.morphDevice(out, VRC_MORPH_DILATE, 100, list_dev, pivot);\n'
           '    world.morphDevice(out, VRC_MORPH_ERODE, 100, list_dev, nullptr, true, false, VRC_COPY_OR, nullptr);\n'
           '    world.dilateBy(line);\n'
           '    world.erodeBy(V::elementCross());\n'
           '    world.erodeBy(box, true);\n'
           '    world.openBy(ball);\n'
           '    world.closeBy(ball);\n'
           '    world.fitsAt(out, box);\n'
           '    world.match(out, V::elementCross(), V::reflect(line), true);\n'
           '    return ball.size() + box.size();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
