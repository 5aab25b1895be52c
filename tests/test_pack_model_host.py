"""The sparse tile stream without a GPU: the numpy model (pack_model.py) round trips and names the rule every corruption
breaks, a 4^3 stream written out byte by byte, vrc_pack_bound and vrc_pack_header against the model, and the refusals of
the two volume calls that precede a device call."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import pack_model as model
from volume_support import ROOT, check_cpp_syntax


@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_model_round_trip_and_corruptions(depth):
    seen = set()
    for name, field in model.fields(depth):
        stream = model.pack(field, depth)
        assert model.header_rule(stream) is None and len(stream) % 4 == 0 and len(stream) <= model.bound(depth)
        back = model.unpack(stream, depth)
        assert isinstance(back, np.ndarray) and np.array_equal(back, field), (depth, name)
        assert model.pack(back, depth) == stream
        h = model.header_of(stream)
        assert h[8] | (h[9] << 32) == int(field.sum())
        if name in ("empty", "full"):
            assert h[4] == h[5] == 0 and len(stream) == 64 + 4 * model.Shape(depth).CW          # B, C and D are absent
        if name == "whole bricks":
            assert h[4] > 0 and h[5] == 0
        if name.startswith("P % 4"):
            assert h[5] % 4 == int(name[-1])
        for rule, variant, bad, where in model.corruptions(stream):
            assert model.unpack(bad, depth) == (rule, where), (depth, name, rule, variant)
            seen.add(rule)
    assert seen == set(model.RULES) - (set() if depth == 2 else {"mask-range"})


def test_depth_2_stream_by_hand():
    """4^3: one tile of K = 8 bricks, q = 4 cx + 2 cy + cz; bricks 0 full, 1 empty, 2 = voxel (0, 2, 0) alone, 5 = voxels (3, 0, 2)
    and (3, 1, 3), the rest empty"""
    solid = np.zeros((4, 4, 4), np.uint8)
    solid[0:2, 0:2, 0:2] = 1                                  # brick (0, 0, 0), q = 0: 0xff
    solid[0, 2, 0] = 1                                        # brick (0, 1, 0), q = 2: bit 0
    solid[3, 0, 2] = 1                                        # brick (1, 0, 1), q = 5: bit (0) 4 + (0) 2 + 1 = 1 -> 0x02
    solid[3, 1, 3] = 1                                        # the same brick: bit (1) 4 + (1) 2 + 1 = 7 -> 0x80
    want = b"".join([
        b"VRCP", struct.pack("<I", 1), struct.pack("<I", 2), struct.pack("<I", 1),      # magic, version, depth, NT
        struct.pack("<I", 1), struct.pack("<I", 2),                                     # M, P
        struct.pack("<Q", 84), struct.pack("<Q", 11), struct.pack("<I", 0), bytes(20),  # length, solid, full tiles, reserved
        struct.pack("<I", 2),                                                           # A: tile 0 is mixed
        struct.pack("<I", 2),                                                           # B: two partial bricks
        struct.pack("<I", 0b00100101), struct.pack("<I", 0b00000001),                   # C: some = q 0, 2, 5; full = q 0
        bytes([0x01, 0x82, 0, 0])])                                                     # D: q 2, q 5, two bytes of padding
    assert len(want) == 84
    assert model.pack(solid, 2) == want
    assert np.array_equal(model.unpack(want, 2), solid)


def test_pack_bound(built):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    for depth in range(2, 11):
        n = 1 << (depth - 1)
        E = min(8, n)
        NT, K = (n // E) ** 3, E ** 3
        formula = 64 + 4 * ((NT + 15) // 16) + 4 * NT + 8 * max(1, K // 32) * NT + 4 * ((n ** 3 + 3) // 4)
        assert L.vrc_pack_bound(depth) == formula == model.bound(depth), depth
    assert L.vrc_pack_bound(2) == 64 + 4 + 4 + 8 + 8 and L.vrc_pack_bound(9) == 21110848
    for depth in (0, 1, 11, 0xFFFFFFFF):
        assert L.vrc_pack_bound(depth) == 0


def header_call(stream, n_bytes=None):
    """(rc, last error, info) of vrc_pack_header over the first 64 bytes of `stream`"""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    head = np.zeros(64, np.uint8)
    head[:min(64, len(stream))] = np.frombuffer(stream[:64], np.uint8)
    info = capi.PackInfo()
    rc = L.vrc_pack_header(capi.ptr(head), len(stream) if n_bytes is None else n_bytes, C.byref(info))
    return rc, L.vrc_last_error().decode(), info


def test_pack_header_against_the_model(built):
    from cpuvoxelraycaster_amd import capi
    assert C.sizeof(capi.PackInfo) == 40
    assert [getattr(capi.PackInfo, k).offset for k in ("depth", "tiles", "mixed_tiles", "full_tiles", "partial_bricks", "reserved", "bytes", "solid")] == \
        [0, 4, 8, 12, 16, 20, 24, 32]
    for depth in (2, 3, 5, 6):
        for name, field in model.fields(depth):
            stream = model.pack(field, depth)
            rc, _, info = header_call(stream)
            h = model.header_of(stream)
            assert rc == 0, (depth, name)
            assert (info.depth, info.tiles, info.mixed_tiles, info.partial_bricks, info.full_tiles, info.reserved, info.bytes, info.solid) == \
                (depth, h[3], h[4], h[5], h[10], 0, len(stream), int(field.sum())), (depth, name)
            for rule, variant, bad, _ in model.corruptions(stream):
                rc, text, _ = header_call(bad)
                want = model.header_rule(bad)                 # the depth rule without a volume: any depth in 2..10
                if want is None:
                    assert rc == 0, (depth, name, rule, variant, text)     # a device-side rule: the header is in order
                else:
                    assert rc == -1 and text == "vrc_pack_header: rule %s" % want, (depth, name, rule, variant, text)
                if rule in model.HEADER_RULES and not (rule == "depth" and variant == 1):
                    assert want == rule
            for cut in model.boundaries(stream):
                for n_bytes in (cut - 4, cut + 4):
                    rc, text, _ = header_call(stream[:n_bytes] if n_bytes < len(stream) else stream + bytes(4))
                    assert rc == -1 and text == "vrc_pack_header: rule %s" % ("header-short" if n_bytes < 64 else "length-argument"), (depth, name, n_bytes)
    from cpuvoxelraycaster_amd import packed_info
    stream = model.pack(model.fields(5)[1][1], 5)
    for data in (stream, np.frombuffer(stream, np.uint8), bytearray(stream)):
        assert packed_info(data).bytes == len(stream) and packed_info(data).depth == 5


def handle(fill=0):
    return (C.c_uint32 * 128)(*([fill] * 128))


ZERO, BUF, INFO_BYTES = handle(), (C.c_uint32 * 32)(), 40


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


# every refusal of the four entry points that precedes the first HIP call: the WHOLE vrc_last_error() text.  ZERO reads as a
# volume of depth 0 on device 0, so a call that reached the device would fail in another way.  "info": a capi.PackInfo.
REFUSALS = [
    ("vrc_pack_header", (None, 64, "info"), "null argument"),
    ("vrc_pack_header", (p(BUF), 64, None), "null argument"),
    ("vrc_pack_header", (p(BUF), 63, "info"), "rule header-short"),
    ("vrc_pack_header", (p(BUF), 64, "info"), "rule magic-version"),
    ("vrc_pack_volume", (None, p(BUF), 128, "info", 0), "null argument"),
    ("vrc_pack_volume", (p(ZERO), p(BUF), 128, None, 0), "null argument"),
    ("vrc_pack_volume", (p(ZERO), p(BUF), 128, "info", 2), "bad mem kind 2"),
    ("vrc_pack_volume", (p(ZERO), p(BUF), 128, "info", -1), "bad mem kind -1"),
    ("vrc_pack_volume", (p(ZERO), None, 128, "info", 0), "null buffer with capacity 128"),
    ("vrc_pack_volume", (p(ZERO), C.c_void_p(0x1002), 128, "info", 1), "device buffer 0x1002 is not aligned to 4 bytes"),
    ("vrc_unpack_volume", (None, p(BUF), 128, 0), "null argument"),
    ("vrc_unpack_volume", (p(ZERO), None, 128, 0), "null argument"),
    ("vrc_unpack_volume", (p(ZERO), p(BUF), 128, 2), "bad mem kind 2"),
    ("vrc_unpack_volume", (p(ZERO), p(BUF), 128, -3), "bad mem kind -3"),
    ("vrc_unpack_volume", (p(ZERO), C.c_void_p(0x1001), 128, 1), "device buffer 0x1001 is not aligned to 4 bytes"),
    ("vrc_unpack_volume", (p(ZERO), p(BUF), 60, 0), "rule header-short"),
    ("vrc_unpack_volume", (p(ZERO), C.c_void_p(0x1000), 60, 1), "rule header-short"),
    ("vrc_unpack_volume", (p(ZERO), p(BUF), 128, 0), "rule magic-version"),
]


@pytest.mark.parametrize("index", range(len(REFUSALS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(REFUSALS)])
def test_pack_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    name, args, text = REFUSALS[index]
    info = capi.PackInfo()
    args = tuple(C.byref(info) if isinstance(a, str) and a == "info" else a for a in args)
    assert getattr(L, name)(*args) == -1                                     # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
    assert not any(ZERO) and not any(BUF) and bytes(info) == bytes(INFO_BYTES)   # nothing was written


def test_every_pack_entry_point_has_its_refusals():
    from cpuvoxelraycaster_amd import capi
    shards = {"vrc_pack_shard", "vrc_unpack_shards"}         # the frame exchange's calls: another family
    assert {n for n in capi.SYMBOLS if "pack_" in n} - shards == {c[0] for c in REFUSALS} | {"vrc_pack_bound"}


def test_host_adapter_with_pack_compiles(built):
    """HipVoxelVolume::pack / packInfo / unpack / save / load in the header-only adapter: C++14, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world) {\n'
           '    const vrc_pack_info info = world.packInfo();\n'
           '    std::vector<uint8_t> stream = world.pack();\n'
           '    world.unpack(stream);\n'
           '    world.unpack(stream.data(), stream.size());\n'
           '    world.save("world.vrcp");\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> other = vrc_host::HipVoxelVolume::load("world.vrcp");\n'
           '    return info.bytes + other->solidCount();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
