"""Volume deltas without a GPU: the numpy model (delta_model.py) against the definition of include/vrc.h taken literally,
the stats struct's layout, every refusal that precedes a device call, and the C++ adapter's new classes."""
import ctypes as C
import os

import numpy as np
import pytest

import delta_model as model
from volume_support import ROOT, check_cpp_syntax


def literal_delta(a, b):
    """records and stats of two [x, y, z] occupancies by the header's words: every voxel's key in Python integers"""
    S = a.shape[0]
    n = S // 2
    bits = {}
    lo, hi, voxels = [S, S, S], [0, 0, 0], 0
    for x in range(S):
        for y in range(S):
            for z in range(S):
                if bool(a[x, y, z]) == bool(b[x, y, z]):
                    continue
                B = ((x >> 1) * n + (y >> 1)) * n + (z >> 1)
                key = 8 * B + (z & 1) * 4 + (y & 1) * 2 + (x & 1)
                bits[key >> 5] = bits.get(key >> 5, 0) | (1 << (key & 31))
                voxels += 1
                for axis, c in enumerate((x, y, z)):
                    lo[axis], hi[axis] = min(lo[axis], c), max(hi[axis], c + 1)
    records = sorted(bits.items())
    if not records:
        lo = hi = [0, 0, 0]
    return records, (len(records), voxels, tuple(lo), tuple(hi), (0, 0))


def literal_words(a):
    S = a.shape[0]
    n = S // 2
    words = [0] * (S ** 3 // 32)
    for x, y, z in np.argwhere(a).tolist():
        key = 8 * (((x >> 1) * n + (y >> 1)) * n + (z >> 1)) + (z & 1) * 4 + (y & 1) * 2 + (x & 1)
        words[key >> 5] |= 1 << (key & 31)
    return words


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_model_is_the_definition(depth):
    S = 1 << depth
    rng = np.random.default_rng(40 + depth)
    for density, flips in [(0.5, 0.01), (0.02, 0.2), (0.98, 0.001), (0.0, 0.0), (0.0, 1.0)]:
        a = (rng.random((S, S, S)) < density).astype(np.uint8)
        b = a ^ (rng.random((S, S, S)) < flips).astype(np.uint8)
        wa, wb = model.words_of(a), model.words_of(b)
        assert wa.dtype == np.uint32 and len(wa) == S ** 3 // 32
        assert wa.tolist() == literal_words(a) and wb.tolist() == literal_words(b)
        assert np.array_equal(model.dense_of(wa, depth), a) and np.array_equal(model.dense_of(wb, depth), b)
        records, stats = model.diff(wa, wb, depth)
        want_records, want_stats = literal_delta(a, b)
        assert list(zip(records["word"].tolist(), records["bits"].tolist())) == want_records
        assert model.stats_tuple(stats) == want_stats
        # apply: before -> after, after -> before, and onto nothing the changed set
        assert np.array_equal(model.apply(wa, records), wb) and np.array_equal(model.apply(wb, records), wa)
        assert np.array_equal(model.apply(model.apply(wa, records), records), wa)
        assert np.array_equal(model.dense_of(model.apply(np.zeros_like(wa), records), depth), a ^ b)


def test_model_single_voxels_at_depth_2():
    """4^3: a word holds the two brick rows cy = 0, 1 of one cx; the boxes by hand"""
    for voxel, word, bit in [((0, 0, 0), 0, 0), ((1, 3, 2), 0, 16 + 8 + 2 + 1), ((2, 1, 3), 1, 8 + 4 + 2), ((3, 3, 3), 1, 31)]:
        a = np.zeros((4, 4, 4), np.uint8)
        b = a.copy()
        b[voxel] = 1
        records, stats = model.diff(model.words_of(a), model.words_of(b), 2)
        assert records.tolist() == [(word, 1 << bit)]
        assert model.stats_tuple(stats) == (1, 1, voxel, tuple(c + 1 for c in voxel), (0, 0))


def test_delta_struct_layout(built):
    from cpuvoxelraycaster_amd import capi
    S = capi.DeltaStats
    assert C.sizeof(S) == 48
    assert [getattr(S, k).offset for k in ("words", "voxels", "lo", "hi", "reserved")] == [0, 8, 16, 28, 40]
    assert capi.DELTA_RECORD_DTYPE == model.RECORD_DTYPE and capi.DELTA_RECORD_DTYPE.itemsize == 8
    assert [capi.DELTA_RECORD_DTYPE.fields[k][1] for k in ("word", "bits")] == [0, 4]


def test_delta_refusals_need_no_gpu(built):
    """NULLs, before == after, volumes of two depths, a depth outside 2..10 and a bad mem kind are VRC_ERR_INVALID with the
    function's name before any HIP call: the handles here are not volumes or deltas at all, and nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b, c = (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)()    # zero bytes: "depth 0 on device 0, no records"
    for i in range(128):
        c[i] = 0x01010101                                                        # every field differs from a's and b's
    pa, pb, pc = (C.cast(x, C.c_void_p) for x in (a, b, c))
    out, stats = C.c_void_p(0x55), capi.DeltaStats()
    stats.words = 7
    for before, after, o in [(None, pb, C.byref(out)), (pa, None, C.byref(out)), (pa, pb, None), (pa, pa, C.byref(out)), (pa, pc, C.byref(out))]:
        for st in (None, C.byref(stats)):
            assert L.vrc_delta_diff(before, after, o, st) == -1
            assert L.vrc_last_error().startswith(b"vrc_delta_diff"), L.vrc_last_error()
    assert L.vrc_delta_diff(pa, pa, C.byref(out), None) == -1 and b"same volume" in L.vrc_last_error()
    assert L.vrc_delta_diff(pa, pc, C.byref(out), None) == -1 and b"depths" in L.vrc_last_error()

    records = np.array([(0, 1)], capi.DELTA_RECORD_DTYPE)
    for depth in (0, 1, 11, 12, 0xFFFFFFFF):
        assert L.vrc_delta_create(depth, 0, 1, capi.ptr(records), capi.VRC_MEM_HOST, C.byref(out), C.byref(stats)) == -1
        assert L.vrc_last_error().startswith(b"vrc_delta_create: depth"), L.vrc_last_error()
    for mem in (-1, 2, 7):
        assert L.vrc_delta_create(3, 0, 1, capi.ptr(records), mem, C.byref(out), None) == -1
        assert b"bad mem kind" in L.vrc_last_error()
    assert L.vrc_delta_create(3, 0, 1, capi.ptr(records), capi.VRC_MEM_HOST, None, None) == -1
    assert L.vrc_delta_create(3, 0, 1, None, capi.VRC_MEM_HOST, C.byref(out), None) == -1
    assert L.vrc_last_error().startswith(b"vrc_delta_create: null records"), L.vrc_last_error()

    assert L.vrc_delta_destroy(None) == 0
    assert L.vrc_delta_count(None) == 0 and L.vrc_delta_depth(None) == 0 and L.vrc_delta_bytes(None) == 0
    assert L.vrc_delta_get_stats(None, C.byref(stats)) == -1 and L.vrc_delta_get_stats(pa, None) == -1
    buf = np.full(4, 9, np.uint32)
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_delta_records(None, 0, 2, capi.ptr(buf), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_delta_records")
        assert L.vrc_delta_records(pa, 0, 2, capi.ptr(buf), mem, None) == 0          # no records: nothing to copy, no device call
    for mem in (-1, 2):
        assert L.vrc_delta_records(pa, 0, 2, capi.ptr(buf), mem, None) == -1 and b"bad mem kind" in L.vrc_last_error()
    assert L.vrc_delta_records(pa, 0, 2, None, capi.VRC_MEM_HOST, None) == -1        # capacity without a buffer
    assert L.vrc_delta_apply(None, pb, None) == -1 and L.vrc_delta_apply(pa, None, None) == -1
    assert L.vrc_last_error().startswith(b"vrc_delta_apply")
    assert L.vrc_delta_apply(pa, pc, None) == -1                                     # a volume of another depth (and device)
    assert L.vrc_last_error().startswith(b"vrc_delta_apply: delta of depth"), L.vrc_last_error()
    assert L.vrc_delta_apply(pa, pb, None) == 0                                      # an empty delta: a no-op before any device call
    assert out.value == 0x55 and stats.words == 7 and np.all(buf == 9)
    assert not any(a) and not any(b) and all(v == 0x01010101 for v in c)


def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


# `device` is the first member and `depth` the second of a vrc_delta; a volume's depth is its third 32-bit word
ZERO, OTHER, ONES, DEVICE_1 = handle(), handle(), handle(0x01010101), handle(w0=1)
OUT, BUF = C.c_void_p(0x55), (C.c_uint32 * 8)()


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


# every refusal of the vrc_delta_* entry points that precedes the first HIP call: the WHOLE vrc_last_error() text, as literals
REFUSALS = [
    ("vrc_delta_diff", (None, p(OTHER), C.byref(OUT), None), "null argument"),
    ("vrc_delta_diff", (p(ZERO), None, C.byref(OUT), None), "null argument"),
    ("vrc_delta_diff", (p(ZERO), p(OTHER), None, None), "null argument"),
    ("vrc_delta_diff", (p(ZERO), p(ZERO), C.byref(OUT), None), "before and after are the same volume"),
    ("vrc_delta_diff", (p(ZERO), p(ONES), C.byref(OUT), None), "volumes of depths 0 and 16843009"),
    ("vrc_delta_diff", (p(ZERO), p(DEVICE_1), C.byref(OUT), None), "volumes on devices 0 and 1"),
    ("vrc_delta_create", (3, 0, 1, p(BUF), 0, None, None), "null argument"),
    ("vrc_delta_create", (1, 0, 1, p(BUF), 0, C.byref(OUT), None), "depth 1 not in [2,10]"),
    ("vrc_delta_create", (11, 0, 0, None, 1, C.byref(OUT), None), "depth 11 not in [2,10]"),
    ("vrc_delta_create", (3, 0, 1, p(BUF), 2, C.byref(OUT), None), "bad mem kind 2"),
    ("vrc_delta_create", (3, 0, 1, p(BUF), -1, C.byref(OUT), None), "bad mem kind -1"),
    ("vrc_delta_create", (3, 0, 5, None, 1, C.byref(OUT), None), "null records with n = 5"),
    ("vrc_delta_get_stats", (None, "stats"), "null argument"),             # "stats": a capi.DeltaStats, made in the test
    ("vrc_delta_get_stats", (p(ZERO), None), "null argument"),
    ("vrc_delta_records", (None, 0, 1, p(BUF), 0, None), "null delta"),
    ("vrc_delta_records", (p(ZERO), 0, 1, p(BUF), 2, None), "bad mem kind 2"),
    ("vrc_delta_records", (p(ZERO), 0, 3, None, 1, None), "null buffer with capacity 3"),
    ("vrc_delta_apply", (None, p(OTHER), None), "null argument"),
    ("vrc_delta_apply", (p(ZERO), None, None), "null argument"),
    ("vrc_delta_apply", (p(ZERO), p(ONES), None), "delta of depth 0, volume of depth 16843009"),
    ("vrc_delta_apply", (p(ZERO), p(DEVICE_1), None), "delta on device 0, volume on device 1"),
    # two refusals at once: the one that wins
    ("vrc_delta_diff", (p(ZERO), p(ZERO), None, None), "null argument"),
    ("vrc_delta_diff", (p(ONES), p(DEVICE_1), C.byref(OUT), None), "volumes of depths 16843009 and 0"),
    ("vrc_delta_diff", (p(DEVICE_1), p(ONES), C.byref(OUT), None), "volumes of depths 0 and 16843009"),
]


@pytest.mark.parametrize("index", range(len(REFUSALS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(REFUSALS)])
def test_delta_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    name, args, text = REFUSALS[index]
    stats = capi.DeltaStats()
    args = tuple(C.byref(stats) if a == "stats" else a for a in args)
    assert getattr(L, name)(*args) == -1                                     # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
    # nothing was written through any handle or buffer
    assert not any(ZERO) and not any(OTHER) and all(v == 0x01010101 for v in ONES) and list(DEVICE_1) == [1] + [0] * 127
    assert not any(BUF) and OUT.value == 0x55 and bytes(stats) == bytes(48)


def test_every_delta_entry_point_has_its_refusals():
    from cpuvoxelraycaster_amd import capi
    silent = {"vrc_delta_destroy", "vrc_delta_count", "vrc_delta_depth", "vrc_delta_bytes"}     # a null handle is 0 / a no-op
    assert {n for n in capi.SYMBOLS if n.startswith("vrc_delta_")} == {c[0] for c in REFUSALS} | silent


def test_delta_without_a_device_fails_loudly(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import cpuvoxelraycaster_amd as vrc
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    out = C.c_void_p(0x55)
    records = np.array([(0, 1)], capi.DELTA_RECORD_DTYPE)
    for n, p in [(1, capi.ptr(records)), (0, None)]:
        assert L.vrc_delta_create(3, 0, n, p, capi.VRC_MEM_HOST, C.byref(out), None) == -2
    assert out.value == 0x55
    with pytest.raises(vrc.VrcError):
        vrc.VoxelDelta.fromRecords(3, records)


def test_host_adapter_with_deltas_compiles(built):
    """HipVoxelDelta, HipVoxelVolume::diff / applyDelta and HipVoxelHistory in the header-only adapter: C++14, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world) {\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> before = world.clone();\n'
           '    world.fillBox(1, 2, 3, 4, 5, 6, false);\n'
           '    vrc_host::HipVoxelDelta delta = before->diff(world);\n'
           '    before->applyDelta(delta);\n'
           '    vrc_host::HipVoxelDelta moved = std::move(delta);\n'
           '    const vrc_delta_stats stats = moved.stats();\n'
           '    vrc_host::HipVoxelDelta copy = vrc_host::HipVoxelDelta::fromRecords(moved.depth(), moved.records(0, 4));\n'
           '    vrc_host::HipVoxelHistory history(world, 1 << 20);\n'
           '    const vrc_host::HipVoxelDelta* step = history.record();\n'
           '    step = history.undo();\n'
           '    step = history.redo();\n'
           '    return stats.voxels + copy.count() + copy.bytes() + history.bytes() + history.undoCount() + history.redoCount() + (step ? 1 : 0);\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
