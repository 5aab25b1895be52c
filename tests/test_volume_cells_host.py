"""The cell calls without a GPU: the numpy model (cells_model.py) against the rules of include/vrc.h taken literally in Python
integers, the coverage of the three-band field the GPU tests count on, every refusal that precedes a device call by its
whole text, the symbols, and the C++ adapter's new methods."""
import ctypes as C
import os

import numpy as np
import pytest

import cells_model as model
from volume_support import ROOT, check_cpp_syntax

M32 = 0xFFFFFFFF


def literal_L(u):
    u ^= u >> 16
    u = (u * 0x7feb352d) & M32
    u ^= u >> 15
    u = (u * 0x846ca68b) & M32
    u ^= u >> 16
    return u


def literal_hash(seed, x, y, z):
    return literal_L(literal_L(literal_L(literal_L(seed) ^ x) ^ y) ^ z)


def literal_step(vol, neighbours, birth, survive, outside):
    """the header's rule voxel by voxel: (dst as nested lists, the counts, changed)"""
    S = len(vol)
    dst = [[[0] * S for _ in range(S)] for _ in range(S)]
    cnt = [[[0] * S for _ in range(S)] for _ in range(S)]
    changed = 0
    for x in range(S):
        for y in range(S):
            for z in range(S):
                c = 0
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dz in (-1, 0, 1):
                            shared = abs(dx) + abs(dy) + abs(dz)          # 1: a face, 2: an edge, 3: a corner
                            if shared == 0 or (neighbours == 6 and shared != 1):
                                continue
                            q = (x + dx, y + dy, z + dz)
                            c += vol[q[0]][q[1]][q[2]] if min(q) >= 0 and max(q) < S else outside
                cnt[x][y][z] = c
                dst[x][y][z] = (survive >> c) & 1 if vol[x][y][z] else (birth >> c) & 1
                changed += dst[x][y][z] != vol[x][y][z]
    return dst, cnt, changed


@pytest.mark.parametrize("S", [4, 8])
def test_model_step_is_the_header(S):
    rng = np.random.default_rng(60 + S)
    fields = [model.three_band(S), (rng.random((S, S, S)) < 0.5).astype(np.uint8), np.zeros((S, S, S), np.uint8), np.ones((S, S, S), np.uint8)]
    for vol in fields:
        for neighbours in (6, 26):
            for outside in (0, 1):
                legal = (2 << neighbours) - 1
                birth, survive = int(rng.integers(0, 1 << 32)) & legal, int(rng.integers(0, 1 << 32)) & legal
                want, cnt, changed = literal_step(vol.tolist(), neighbours, birth, survive, outside)
                assert model.counts(vol, neighbours, outside).tolist() == cnt
                got, got_changed = model.step(vol, birth, survive, neighbours, outside)
                assert got.dtype == np.uint8 and got.tolist() == want and got_changed == changed


@pytest.mark.parametrize("S", [4, 8])
def test_model_hash_is_the_header(S):
    assert [int(v) for v in model.finalise(np.array([0, 1, 7, 0x80000000, M32], np.uint32))] == [literal_L(v) for v in (0, 1, 7, 0x80000000, M32)]
    for seed in (0, 7, 0xDEADBEEF, M32):
        want = [[[literal_hash(seed, x, y, z) for z in range(S)] for y in range(S)] for x in range(S)]
        assert model.hash_field(seed, S).tolist() == want
        for threshold in (0, 1, 1 << 31, model.threshold_of(0.12), M32, 1 << 32):
            selected = [[[int(h < threshold) for h in row] for row in plane] for plane in want]
            assert model.random_set(seed, threshold, S).tolist() == selected
    assert model.random_set(3, 0, S).sum() == 0 and model.random_set(3, 1 << 32, S).sum() == S ** 3
    # the field does not depend on the depth or on the box
    assert np.array_equal(model.hash_field(7, 2 * S)[:S, :S, :S], model.hash_field(7, S))
    vol = np.ones((S, S, S), np.uint8)
    box = (1, 0, 1, S - 1, S, 3)
    got = model.fill_random(vol, 5, 1 << 31, box, model.ANDNOT)
    R = model.random_set(5, 1 << 31, S)
    inside = np.zeros((S, S, S), bool)
    inside[1:S - 1, :, 1:3] = True
    assert np.array_equal(got, np.where(inside, 1 - R, 1))
    assert np.array_equal(model.fill_random(vol, 5, 1 << 31, (3, 3, 3, 3, 4, 4), model.REPLACE), vol)      # an empty box
    assert model.threshold_of(0.0) == 0 and model.threshold_of(1.0) == 1 << 32 and model.threshold_of(0.5) == 1 << 31


def test_model_wrappers_by_hand():
    vol = np.zeros((8, 8, 8), np.uint8)
    vol[2:6, 2:6, 2:6] = 1
    vol[0, 0, 0] = vol[7, 3, 3] = 1                            # two specks
    vol[3, 3, 3] = 0                                           # a pin-hole
    cleaned = model.remove_specks(vol)
    assert cleaned[0, 0, 0] == 0 and cleaned[7, 3, 3] == 0 and cleaned.sum() == vol.sum() - 2
    smoothed = model.smooth(vol)
    assert smoothed[3, 3, 3] == 1 and smoothed[0, 0, 0] == 0 and smoothed[2, 2, 2] == 0      # hole filled, speck gone, corner rounded
    assert model.SMOOTH_BIRTH == 0x7FFC000 and model.SMOOTH_SURVIVE == 0x7FFE000 and model.SPECKS_SURVIVE == 0x7E
    state, taken = model.automaton(vol, 50, 0, model.SPECKS_SURVIVE, 6, 0)
    assert taken == 1 and np.array_equal(state, cleaned)       # the second step changes nothing


@pytest.mark.parametrize("S", [16, 32])
def test_three_band_field_reaches_every_count(S):
    """What the single-count GPU cases rest on: at 16^3 and 32^3 the field holds a solid and an empty voxel with every count
    0 .. N, for both neighbourhoods and both values of outside.  (At 4^3 and 8^3 it does not: those sizes prove the branches,
    not the completeness.)"""
    vol = model.three_band(S)
    for neighbours in (6, 26):
        for outside in (0, 1):
            c = model.counts(vol, neighbours, outside)
            for solid in (0, 1):
                assert set(np.unique(c[vol == solid]).tolist()) == set(range(neighbours + 1)), (S, neighbours, outside, solid)


def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


# `device` is the first 32-bit word of a vrc_volume and `depth` its third
ZERO, OTHER, DEPTH_3, DEVICE_1 = handle(), handle(), handle(w2=3), handle(w0=1)
CHANGED, BOX = C.c_uint64(0x55), (C.c_uint32 * 6)(5, 5, 5, 2, 2, 2)


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


def step_args(dst=ZERO, src=OTHER, neighbours=26, birth=0, survive=0, outside=0, changed=None, mem=0):
    return (p(dst), p(src), neighbours, birth, survive, outside, changed, mem, None)


# every refusal of the vrc_cells_* entry points, all before the first HIP call: the WHOLE vrc_last_error() text, as literals
REFUSALS = [
    ("vrc_cells_step", step_args(dst=None), "null argument"),
    ("vrc_cells_step", step_args(src=None), "null argument"),
    ("vrc_cells_step", step_args(src=ZERO), "source and destination are the same volume"),
    ("vrc_cells_step", step_args(src=DEPTH_3), "volumes of depths 0 and 3"),
    ("vrc_cells_step", step_args(src=DEVICE_1), "volumes on devices 0 and 1"),
    ("vrc_cells_step", step_args(neighbours=18), "neighbours 18 is neither 6 nor 26"),
    ("vrc_cells_step", step_args(neighbours=0), "neighbours 0 is neither 6 nor 26"),
    ("vrc_cells_step", step_args(neighbours=27), "neighbours 27 is neither 6 nor 26"),
    ("vrc_cells_step", step_args(neighbours=-6), "neighbours -6 is neither 6 nor 26"),
    ("vrc_cells_step", step_args(birth=1 << 27), "birth_mask 0x8000000 has a bit above bit 26"),
    ("vrc_cells_step", step_args(neighbours=6, birth=0x80), "birth_mask 0x80 has a bit above bit 6"),
    ("vrc_cells_step", step_args(survive=0x80000001), "survive_mask 0x80000001 has a bit above bit 26"),
    ("vrc_cells_step", step_args(neighbours=6, birth=0x7F, survive=0x4000), "survive_mask 0x4000 has a bit above bit 6"),
    ("vrc_cells_step", step_args(outside=2), "outside 2 is neither 0 nor 1"),
    ("vrc_cells_step", step_args(outside=-1), "outside -1 is neither 0 nor 1"),
    ("vrc_cells_step", step_args(changed=C.byref(CHANGED), mem=2), "bad mem kind 2"),
    ("vrc_cells_step", step_args(changed=C.byref(CHANGED), mem=-1), "bad mem kind -1"),
    ("vrc_cells_fill_random", (None, 1, 1 << 31, None, 1, None), "null volume"),
    ("vrc_cells_fill_random", (p(ZERO), 1, (1 << 32) + 1, None, 1, None), "threshold 4294967297 above 2^32"),
    ("vrc_cells_fill_random", (p(ZERO), 1, M32 << 32, p(BOX), 0, None), "threshold 18446744069414584320 above 2^32"),
    ("vrc_cells_fill_random", (p(ZERO), 1, 1 << 32, None, 3, None), "bad op 3"),
    ("vrc_cells_fill_random", (p(ZERO), 1, 0, p(BOX), -1, None), "bad op -1"),
    # two refusals at once: the one that wins
    ("vrc_cells_step", step_args(src=ZERO, neighbours=18), "source and destination are the same volume"),
    ("vrc_cells_step", step_args(src=DEPTH_3, dst=DEVICE_1), "volumes of depths 0 and 3"),
    ("vrc_cells_step", step_args(src=DEPTH_3, outside=2), "volumes of depths 0 and 3"),
    ("vrc_cells_step", step_args(src=DEVICE_1, neighbours=0), "volumes on devices 0 and 1"),
    ("vrc_cells_step", step_args(dst=DEVICE_1, changed=C.byref(CHANGED), mem=2), "volumes on devices 1 and 0"),
]


def untouched():
    return (not any(ZERO) and not any(OTHER) and list(DEPTH_3) == [0, 0, 3] + [0] * 125 and list(DEVICE_1) == [1] + [0] * 127
            and CHANGED.value == 0x55 and list(BOX) == [5, 5, 5, 2, 2, 2])


@pytest.mark.parametrize("index", range(len(REFUSALS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(REFUSALS)])
def test_cells_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    name, args, text = REFUSALS[index]
    assert getattr(L, name)(*args) == -1                                     # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
    assert untouched()                                                       # nothing was written through any handle or buffer


def test_empty_box_is_a_no_op_before_any_device_call(built):
    """the handle is no volume at all ("depth 0": one voxel): an inverted box, an empty one and one wholly outside return
    VRC_OK without a device call"""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    for box in [(5, 5, 5, 2, 2, 2), (0, 0, 0, 1, 0, 1), (1, 0, 0, 4, 4, 4)]:
        for op in (0, 1, 2):
            assert L.vrc_cells_fill_random(p(ZERO), 9, 1 << 31, p((C.c_uint32 * 6)(*box)), op, None) == 0
    assert untouched()


def test_every_cells_entry_point_has_its_refusals():
    from cpuvoxelraycaster_amd import capi
    names = {n for n in capi.SYMBOLS if n.startswith("vrc_cells_")}
    assert names == {"vrc_cells_step", "vrc_cells_fill_random"} == {c[0] for c in REFUSALS}
    assert not any(n.startswith("vrc_volume_") for n in names)
    assert (capi.VRC_CELLS_FACES, capi.VRC_CELLS_ALL) == (6, 26)


def test_wrappers_and_exports():
    import cpuvoxelraycaster_amd as vrc
    for name in ("cellStep", "cellStepDevice", "automaton", "smooth", "removeSpecks", "fillRandom", "caves"):
        assert callable(getattr(vrc.VoxelVolume, name)), name
    assert "count_mask" in vrc.__all__
    assert vrc.count_mask(range(14, 27)) == model.SMOOTH_BIRTH and vrc.count_mask(range(13, 27)) == model.SMOOTH_SURVIVE
    assert vrc.count_mask(0x7E) == 0x7E == vrc.count_mask([1, 2, 3, 4, 5, 6]) and vrc.count_mask([]) == 0
    assert vrc.VoxelVolume.countMask(np.uint32(5)) == 5


def test_host_adapter_with_cells_compiles(built):
    """HipVoxelVolume::cellStep / automaton / smooth / removeSpecks / fillRandom / caves in the header-only adapter: C++14, no
    HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& next) {\n'
           '    uint64_t changed = 0;\n'
           '    const uint32_t box[6] = {1, 2, 3, 9, 8, 7};\n'
           '    world.fillRandom(7, 0.45);\n'
           '    world.fillRandom(7, 0.45, box, VRC_COPY_ANDNOT);\n'
           '    world.cellStep(next, 1u << 5, 0x7E0u, VRC_CELLS_ALL, true, &changed);\n'
           '    world.cellStep(next, 1u << 3, 0x7Eu, VRC_CELLS_FACES);\n'
           '    const uint32_t taken = world.automaton(5, 1u << 5, 0x7E0u);\n'
           '    world.smooth();\n'
           '    world.smooth(3, true);\n'
           '    world.removeSpecks();\n'
           '    world.caves(1337, 0.5, 4);\n'
           '    return changed + taken;\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
