"""The column calls without a GPU: the numpy model (columns_model.py) pinned against tiny cases worked out by hand and against
the header's rules taken literally voxel by voxel, every refusal that precedes a device call by its whole text, the symbols,
and the C++ adapter's new methods."""
import ctypes as C
import os

import numpy as np
import pytest

import columns_model as model
from volume_support import ROOT, check_cpp_syntax

NONE = 0xFFFFFFFF


def column(bits):
    """a 4^3 volume that is empty but for column (u, v) = (1, 2) along z, solid where bits[z]"""
    vol = np.zeros((4, 4, 4), np.uint8)
    vol[1, 2, :] = bits
    return vol


def test_profile_by_hand():
    vol = column([0, 1, 0, 1])
    up, down = model.profile(vol, 5), model.profile(vol, 4)                    # along z: towards larger / smaller z
    assert up.shape == (4, 4) and up.dtype.itemsize == 16
    assert tuple(up[1, 2]) == (1, 3, 2, 2) and tuple(down[1, 2]) == (3, 1, 2, 2)
    assert tuple(up[0, 0]) == (NONE, NONE, 0, 0) and (up["count"].sum(), up["runs"].sum()) == (2, 2)
    assert tuple(model.profile(column([1, 1, 1, 0]), 5)[1, 2]) == (0, 2, 3, 1)
    assert tuple(model.profile(column([1, 1, 1, 1]), 4)[1, 2]) == (3, 0, 4, 1)
    # the same voxels seen along x and y: two columns of one voxel each; (u, v) = (y, z) and (x, z)
    along_x, along_y = model.profile(vol, 1), model.profile(vol, 2)
    assert tuple(along_x[2, 1]) == (1, 1, 1, 1) and tuple(along_x[2, 3]) == (1, 1, 1, 1) and along_x["count"].sum() == 2
    assert tuple(along_y[1, 1]) == (2, 2, 1, 1) and tuple(along_y[1, 3]) == (2, 2, 1, 1) and along_y["count"].sum() == 2
    # a rect is a window of the whole map
    assert np.array_equal(model.profile(vol, 5, (1, 1, 3, 4)), up[1:3, 1:4]) and model.profile(vol, 5, (1, 2, 2, 3)).shape == (1, 1)
    assert model.height_map(vol, 4)[1, 2] == 3 and model.height_map(vol, 4, -9)[0, 0] == -9 and model.thickness_map(vol, 2)[1, 2] == 2
    assert not model.is_height_field(vol, 4) and model.is_height_field(column([0, 1, 1, 0]), 4)
    assert not model.is_height_field(column([0, 1, 1, 0]), 4, grounded=True) and model.is_height_field(column([1, 1, 0, 0]), 4, grounded=True)
    assert model.is_height_field(column([0, 0, 1, 1]), 5, grounded=True) and not model.is_height_field(column([1, 1, 0, 0]), 5, grounded=True)
    assert [model.profile(model.alternating(8, a, ph), 2 * a)["runs"].min() for a in (0, 1, 2) for ph in (0, 1)] == [4] * 6


def test_fill_by_hand():
    I = np.iinfo(np.int32)
    full = np.ones((4, 4, 4), np.uint8)
    got = model.fill(full, 2, 1, 3, (1, 2, 2, 3), model.REPLACE)
    want = full.copy()
    want[1, 2, :] = [0, 1, 1, 0]
    assert np.array_equal(got, want) and full.all()                           # the input is not written
    got = model.fill(full, 2, 1, 3, (1, 2, 2, 3), model.ANDNOT)
    want[1, 2, :] = [1, 0, 0, 1]
    assert np.array_equal(got, want)
    empty = np.zeros((4, 4, 4), np.uint8)
    lo = np.array([[I.min, -1], [2, 3]], np.int32)
    hi = np.array([[1, I.max], [2, 9]], np.int32)
    got = model.fill(empty, 0, lo, hi, (0, 1, 2, 3), model.OR)                 # along x: (u, v) = (y, z)
    want = np.zeros((4, 4, 4), np.uint8)
    want[0:1, 0, 1] = 1                                                        # [-2^31, 1)
    want[:, 0, 2] = 1                                                          # [-1, 2^31 - 1)
    want[3:4, 1, 2] = 1                                                        # [3, 9); [2, 2) is empty
    assert np.array_equal(got, want)
    assert np.array_equal(model.fill(empty, 1, 1, 3), np.broadcast_to(np.array([0, 1, 1, 0], np.uint8)[None, :, None], (4, 4, 4)))
    h = np.array([[0, 17], [99, 31]])
    t = model.raise_terrain(np.pad(h, ((0, 30), (0, 30))), 5)
    assert [int(t[x, :, z].sum()) for x, z in ((0, 0), (0, 1), (1, 0), (1, 1), (5, 5))] == [15, 15, 15, 15, 15]      # 17 .. 31, cut at S
    t = model.raise_terrain(np.full((64, 64), 20), 6)
    assert t[3, :, 4].tolist() == [0] * 33 + [1] * 19 + [0] * 12


def test_select_by_hand():
    vol = column([0, 1, 0, 1])
    assert model.before(vol, 5)[1, 2].tolist() == [0, 0, 1, 1] and model.before(vol, 4)[1, 2].tolist() == [2, 1, 1, 0]
    assert model.selection(vol, 5, 0, 1, model.SOLID)[1, 2].tolist() == [0, 1, 0, 0]
    assert model.selection(vol, 4, 0, 1, model.SOLID)[1, 2].tolist() == [0, 0, 0, 1]
    assert model.selection(vol, 5, 0, 1, model.EMPTY)[1, 2].tolist() == [1, 0, 0, 0]
    assert model.selection(vol, 5, 1, 5, model.EMPTY)[1, 2].tolist() == [0, 0, 1, 0]
    assert model.selection(vol, 4, 1, 2, model.BOTH)[1, 2].tolist() == [0, 1, 1, 0]
    assert model.selection(vol, 5, 0, 2, model.SOLID).sum() == 2 and model.selection(vol, 5, 1, 1, model.BOTH).sum() == 0
    assert model.selection(vol, 5, 0, 1, model.EMPTY).sum() == 64 - 4 + 1      # every other column is open sky
    dst = np.ones((4, 4, 4), np.uint8)
    assert model.select(dst, vol, 5, 0, 1, model.SOLID, model.ANDNOT).sum() == 63 and model.select(dst, vol, 5, 0, 1, model.SOLID).sum() == 1


def literal(vol, direction):
    """the header's definitions voxel by voxel: (records by (u, v), P by (x, y, z))"""
    S = len(vol)
    axis, side = direction >> 1, direction & 1
    others = [a for a in range(3) if a != axis]
    records, P = {}, {}
    for u in range(S):
        for v in range(S):
            first = last = NONE
            count = runs = 0
            previous = 0
            for t in range(S):
                p = [0, 0, 0]
                p[axis], p[others[0]], p[others[1]] = (t if side else S - 1 - t), u, v
                P[tuple(p)] = count
                s = int(vol[p[0]][p[1]][p[2]])
                if s:
                    first = p[axis] if first == NONE else first
                    last = p[axis]
                    count += 1
                    runs += not previous
                previous = s
            records[(u, v)] = (first, last, count, runs)
    return records, P


@pytest.mark.parametrize("S", [4, 8])
def test_model_is_the_header(S):
    rng = np.random.default_rng(70 + S)
    for vol in [(rng.random((S, S, S)) < 0.5).astype(np.uint8), (rng.random((S, S, S)) < 0.1).astype(np.uint8), np.ones((S, S, S), np.uint8)]:
        for direction in model.DIRECTIONS:
            records, P = literal(vol.tolist(), direction)
            got = model.profile(vol, direction)
            assert {(u, v): tuple(int(f) for f in got[u, v]) for u in range(S) for v in range(S)} == records
            before = model.before(vol, direction)
            assert all(before[p] == c for p, c in P.items())
            lo, hi = sorted(int(b) for b in rng.integers(0, S + 2, 2))
            for of in (model.SOLID, model.EMPTY, model.BOTH):
                want = np.zeros((S, S, S), np.uint8)
                for p, c in P.items():
                    want[p] = lo <= c < hi and bool(of & (model.SOLID if vol[p] else model.EMPTY))
                assert np.array_equal(model.selection(vol, direction, lo, hi, of), want)
        for axis in range(3):
            lo, hi = rng.integers(-3, S + 4, (2, S - 1, S - 2))
            rect = (1, 1, S, S - 1)
            for op in (model.REPLACE, model.OR, model.ANDNOT):
                want = vol.copy()
                for u in range(rect[0], rect[2]):
                    for v in range(rect[1], rect[3]):
                        for t in range(S):
                            p = [0, 0, 0]
                            p[axis] = t
                            p[[a for a in range(3) if a != axis][0]], p[[a for a in range(3) if a != axis][1]] = u, v
                            inside = lo[u - 1, v - 1] <= t < hi[u - 1, v - 1]
                            want[tuple(p)] = inside if op == model.REPLACE else (want[tuple(p)] | inside) if op == model.OR else (want[tuple(p)] & (not inside))
                assert np.array_equal(model.fill(vol, axis, lo, hi, rect, op), want), (axis, op)


def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


# `device` is the first 32-bit word of a vrc_volume and `depth` its third
ZERO, OTHER, DEPTH_3, DEVICE_1, DEPTH_1_DEVICE_1 = handle(), handle(), handle(w2=3), handle(w0=1), handle(w0=1, w2=1)
OUT, MAP = (C.c_uint32 * 4)(7, 7, 7, 7), (C.c_int32 * 4)(1, 2, 3, 4)


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


def rect(*r):
    return (C.c_uint32 * 4)(*r)


def profile_args(v=DEPTH_3, direction=2, r=None, out=OUT, mem=0):
    return (p(v), direction, p(r), p(out), mem, None)


def fill_args(v=DEPTH_3, axis=1, r=None, lo_map=None, lo=0, hi_map=None, hi=4, op=1, mem=0):
    return (p(v), axis, p(r), p(lo_map), lo, p(hi_map), hi, op, mem, None)


def select_args(dst=ZERO, src=OTHER, direction=2, lo=0, hi=1, of=1, op=0):
    return (p(dst), p(src), direction, lo, hi, of, op, None)


# every refusal of the vrc_columns_* entry points, all before the first HIP call: the WHOLE vrc_last_error() text, as literals
REFUSALS = [
    ("vrc_columns_profile", profile_args(v=None), "null volume"),
    ("vrc_columns_profile", profile_args(out=None), "null out"),
    ("vrc_columns_profile", profile_args(direction=6), "bad direction 6"),
    ("vrc_columns_profile", profile_args(direction=-1), "bad direction -1"),
    ("vrc_columns_profile", profile_args(r=rect(2, 2, 2, 5)), "rect (2, 2, 2, 5) is empty or outside the 8 x 8 face"),
    ("vrc_columns_profile", profile_args(r=rect(5, 1, 3, 8)), "rect (5, 1, 3, 8) is empty or outside the 8 x 8 face"),
    ("vrc_columns_profile", profile_args(r=rect(0, 0, 9, 8)), "rect (0, 0, 9, 8) is empty or outside the 8 x 8 face"),
    ("vrc_columns_profile", profile_args(r=rect(0, 7, 8, 0xFFFFFFFF)), "rect (0, 7, 8, 4294967295) is empty or outside the 8 x 8 face"),
    ("vrc_columns_profile", profile_args(v=ZERO, r=rect(0, 0, 1, 2)), "rect (0, 0, 1, 2) is empty or outside the 1 x 1 face"),
    ("vrc_columns_profile", profile_args(mem=2), "bad mem kind 2"),
    ("vrc_columns_profile", profile_args(r=rect(1, 1, 8, 8), mem=-1), "bad mem kind -1"),
    ("vrc_columns_fill", fill_args(v=None), "null volume"),
    ("vrc_columns_fill", fill_args(axis=3), "bad axis 3"),
    ("vrc_columns_fill", fill_args(axis=-1), "bad axis -1"),
    ("vrc_columns_fill", fill_args(r=rect(0, 3, 8, 3), lo_map=MAP), "rect (0, 3, 8, 3) is empty or outside the 8 x 8 face"),
    ("vrc_columns_fill", fill_args(r=rect(8, 0, 9, 1)), "rect (8, 0, 9, 1) is empty or outside the 8 x 8 face"),
    ("vrc_columns_fill", fill_args(op=3), "bad op 3"),
    ("vrc_columns_fill", fill_args(op=-1, hi_map=MAP), "bad op -1"),
    ("vrc_columns_fill", fill_args(mem=2), "bad mem kind 2"),
    ("vrc_columns_fill", fill_args(lo_map=MAP, hi_map=MAP, r=rect(0, 0, 2, 2), mem=7), "bad mem kind 7"),
    ("vrc_columns_select", select_args(dst=None), "null argument"),
    ("vrc_columns_select", select_args(src=None), "null argument"),
    ("vrc_columns_select", select_args(src=ZERO), "source and destination are the same volume"),
    ("vrc_columns_select", select_args(src=DEPTH_3), "volumes of depths 0 and 3"),
    ("vrc_columns_select", select_args(src=DEVICE_1), "volumes on devices 0 and 1"),
    ("vrc_columns_select", select_args(direction=6), "bad direction 6"),
    ("vrc_columns_select", select_args(direction=-2), "bad direction -2"),
    ("vrc_columns_select", select_args(lo=5, hi=4), "lo 5 above hi 4"),
    ("vrc_columns_select", select_args(lo=0xFFFFFFFF, hi=0), "lo 4294967295 above hi 0"),
    ("vrc_columns_select", select_args(of=0), "bad of 0"),
    ("vrc_columns_select", select_args(of=4), "bad of 4"),
    ("vrc_columns_select", select_args(op=3), "bad op 3"),
    ("vrc_columns_select", select_args(op=-1), "bad op -1"),
    # two refusals at once: the one that wins
    ("vrc_columns_select", select_args(src=ZERO, direction=6), "source and destination are the same volume"),
    ("vrc_columns_select", select_args(src=DEPTH_1_DEVICE_1), "volumes of depths 0 and 1"),
    ("vrc_columns_select", select_args(src=DEPTH_3, op=3), "volumes of depths 0 and 3"),
    ("vrc_columns_select", select_args(src=DEVICE_1, direction=-2), "volumes on devices 0 and 1"),
    ("vrc_columns_select", select_args(src=DEVICE_1, lo=5, hi=4), "volumes on devices 0 and 1"),
]


def untouched():
    return (not any(ZERO) and not any(OTHER) and list(DEPTH_3) == [0, 0, 3] + [0] * 125 and list(DEVICE_1) == [1] + [0] * 127
            and list(DEPTH_1_DEVICE_1) == [1, 0, 1] + [0] * 125 and list(OUT) == [7] * 4 and list(MAP) == [1, 2, 3, 4])


@pytest.mark.parametrize("index", range(len(REFUSALS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(REFUSALS)])
def test_columns_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    name, args, text = REFUSALS[index]
    assert getattr(L, name)(*args) == -1                                     # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
    assert untouched()                                                       # nothing was written through any handle or buffer


def test_every_columns_entry_point_has_its_refusals():
    from cpuvoxelraycaster_amd import capi
    names = {n for n in capi.SYMBOLS if n.startswith("vrc_columns_")}
    assert names == {"vrc_columns_profile", "vrc_columns_fill", "vrc_columns_select"} == {c[0] for c in REFUSALS}
    assert not any(n.startswith(("vrc_volume_", "vrc_cells_", "vrc_delta_", "vrc_labels_", "vrc_distance_")) or "pack_" in n for n in names)
    assert (capi.VRC_COLUMNS_SOLID, capi.VRC_COLUMNS_EMPTY, capi.VRC_COLUMN_NONE) == (model.SOLID, model.EMPTY, model.NONE)
    assert capi.COLUMN_DTYPE == model.COLUMN_DTYPE and capi.COLUMN_DTYPE.itemsize == 16


def test_wrappers_exist():
    import cpuvoxelraycaster_amd as vrc
    for name in ("columnProfile", "columnProfileDevice", "heightMap", "thicknessMap", "isHeightField", "fillColumns", "fillColumnsDevice", "raiseTerrain",
                 "selectColumns", "skyLit", "topLayers", "sheltered"):
        assert callable(getattr(vrc.VoxelVolume, name)), name


def test_host_adapter_with_columns_compiles(built):
    """HipVoxelVolume::columnProfile / heightMap / thicknessMap / isHeightField / fillColumns / raiseTerrain / selectColumns /
    skyLit / topLayers / sheltered in the header-only adapter: C++14, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& lit) {\n'
           '    const uint32_t rect[4] = {1, 2, 9, 8};\n'
           '    const std::vector<vrc_column> whole = world.columnProfile(2), part = world.columnProfile(5, rect);\n'
           '    const std::vector<int32_t> top = world.heightMap(2), none = world.heightMap(3, -9);\n'
           '    const std::vector<uint32_t> thick = world.thicknessMap(1);\n'
           '    const bool flat = world.isHeightField(2) && world.isHeightField(2, true);\n'
           '    world.fillColumns(1, nullptr, 0, top.data(), 0);\n'
           '    world.fillColumns(0, top.data(), 0, nullptr, 9, nullptr, VRC_COPY_ANDNOT);\n'
           '    world.fillColumnsDevice(2, nullptr, 1, nullptr, 5, rect, VRC_COPY_REPLACE, nullptr);\n'
           '    world.raiseTerrain(top);\n'
           '    world.selectColumns(lit, 2, 0u, 1u, VRC_COLUMNS_SOLID | VRC_COLUMNS_EMPTY, VRC_COPY_OR);\n'
           '    world.skyLit(lit, 2);\n'
           '    world.topLayers(lit, 2, 3);\n'
           '    world.sheltered(lit, 2);\n'
           '    static_assert(sizeof(vrc_column) == 16 && VRC_COLUMN_NONE == 0xffffffffu, "vrc_column");\n'
           '    return whole.size() + part.size() + none.size() + thick.size() + flat;\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
