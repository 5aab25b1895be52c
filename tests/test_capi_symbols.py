"""The C-ABI library loads and exports every symbol include/vrc.h declares; the
product fails loudly (no CPU fallback) when there is no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "vrc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(vrc_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported(built):
    from cpuvoxelraycaster_amd import capi
    lib = C.CDLL(capi.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vrc.h but not exported"
    assert set(names) == set(capi.SYMBOLS), set(names) ^ set(capi.SYMBOLS)


def test_struct_sizes(built):
    from cpuvoxelraycaster_amd import capi
    assert C.sizeof(capi.Camera) == 15 * 4
    assert C.sizeof(capi.FrameParams) == 14 * 4
    assert C.sizeof(capi.FrameStats) == 40
    assert capi.HIT_DTYPE.itemsize == 48 and capi.LNODE_DTYPE.itemsize == 8


def test_host_cpp_mirror_compiles(built):
    """The C++ host adapter mirroring Volumetric / RayCaster compiles against the C ABI."""
    import subprocess
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = '#include "%s"\nint main(){ return 0; }\n' % hdr
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-x", "c++", "-"], input=src.encode(), check=True)


def test_rotation_helper_matches_oracle(built):
    import oracle_lib as O
    from cpuvoxelraycaster_amd import capi
    for ax, ay in [(0.0, 0.0), (0.0, -0.5), (0.3, -1.2), (-2.0, 0.7), (3.0, 1.5)]:
        assert np.array_equal(capi.make_rotation(ax, ay).view(np.uint32), O.make_rotation(ax, ay).view(np.uint32))


def test_no_gpu_fails_loudly(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import cpuvoxelraycaster_amd as vrc
    nodes = np.zeros(9, vrc.LNODE_DTYPE)
    with pytest.raises(vrc.VrcError):
        vrc.LSVO(nodes, 2)
    # ... the frame flags of the peer-write exchange as well: no device, no segment left behind
    f = C.c_void_p()
    L = vrc.capi.load()
    assert L.vrc_ipc_flags_open(b"/vrc_test_no_gpu", 8, 0, 1, C.byref(f)) == -2
    assert not os.path.exists("/dev/shm/vrc_test_no_gpu")


def test_replay_reader_matches_reference_format(built, tmp_path):
    """include/replay.hpp semantics: whitespace-separated ticks, stop at the first malformed one,
    missing file -> empty; the C++ host reader and the Python driver agree."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay_bench
    good = tmp_path / "a.replay"
    good.write_text("0.0 1 2 3 0.1 -0.2\n0.5 4 5 6\n0.3 0.4\n1.0 7 8 9 x 0\n2.0 1 1 1 1 1\n")
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n#include <cstdio>\nint main(int c, char** v){ auto l = vrc_host::readReplay(v[1]);'
           'std::printf("%%zu", l.size()); for (auto& e : l) std::printf(" %%g %%g %%g %%g %%g %%g", e.time, e.pose.position.x, e.pose.position.y, e.pose.position.z, e.pose.view_angle.x, e.pose.view_angle.y);'
           'return 0; }\n') % hdr
    exe = str(tmp_path / "replay_test")
    subprocess.run(["g++", "-std=c++14", "-x", "c++", "-", "-o", exe, "-L" + os.path.join(ROOT, "cpuvoxelraycaster_amd"),
                    "-l:libvrc_hip.so", "-Wl,-rpath," + os.path.join(ROOT, "cpuvoxelraycaster_amd")], input=src.encode(), check=True)
    out = subprocess.run([exe, str(good)], capture_output=True, text=True).stdout.split()
    ticks = replay_bench.load_replay(str(good))
    assert int(out[0]) == len(ticks) == 2
    assert [np.float32(v) for v in out[1:]] == [np.float32(v) for t in ticks for v in t]
    assert subprocess.run([exe, str(tmp_path / "missing")], capture_output=True, text=True).stdout == "0"
    assert replay_bench.load_replay(str(tmp_path / "missing")) == []


def test_argument_validation_needs_no_gpu(built):
    """Bad arguments are refused before any HIP call: depth range, more than VRC_MAX_NODES nodes (the walk addresses a
    node by a 32-bit byte offset), null pointers, bad shard description."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    nodes = np.zeros(8, capi.LNODE_DTYPE)
    h = C.c_void_p()
    assert L.vrc_scene_create(capi.ptr(nodes), (1 << 29) + 1, 9, 0, C.byref(h)) == -1
    assert b"2^29" in L.vrc_last_error()
    assert L.vrc_scene_create(capi.ptr(nodes), 8, 12, 0, C.byref(h)) == -1
    assert L.vrc_scene_create(capi.ptr(nodes), 8, 1, 0, C.byref(h)) == -1
    assert L.vrc_scene_create(None, 8, 9, 0, C.byref(h)) == -1
    assert L.vrc_resolve_shard(None, 8, 0, 1, None, 0, None) == -1
    assert L.vrc_unpack_shards(None, 16, 16, 8, 2, None, None) == -1
    assert L.vrc_shard_bytes(1920, 1080, 8, 8) == 17 * 8 * 1920 * 4
    # direct peer writes / frame flags: bad names and counts, null handles
    f = C.c_void_p()
    assert L.vrc_ipc_flags_open(b"no_slash", 8, 0, 1, C.byref(f)) == -1
    assert L.vrc_ipc_flags_open(b"/vrc_x", 0, 0, 1, C.byref(f)) == -1
    assert L.vrc_ipc_flags_open(None, 8, 0, 1, C.byref(f)) == -1
    assert L.vrc_stream_write_flag(None, 0, 1, None) == -1 and L.vrc_stream_wait_flag(None, 0, 1, None) == -1
    assert L.vrc_ipc_flag_value(None, 0) == 0 and L.vrc_ipc_flags_close(None) == 0 and L.vrc_ipc_flags_unlink(None) == -1
    assert L.vrc_ipc_export_image(None, None) == -1 and L.vrc_ipc_open_image(0, None, None) == -1
    assert L.vrc_renderer_set_image_target(None, None) == -1


def test_bmp_texture_readers(built, tmp_path):
    """The data format in front of the path: the reference loads its two albedo tables from 16 x 16 BMP files
    (raycaster.hpp:53-54).  The host adapter's loadBMP and the Python loader decode a 24-bpp bottom-up file (what the
    reference ships), a 32-bpp one and a top-down one to the same top-down RGB table; the reference's own files (kept under
    tests/golden) decode to the packaged tables."""
    import struct
    import subprocess
    import cpuvoxelraycaster_amd as vrc
    top, side = vrc.load_textures()
    rgb = top.reshape(16, 16, 3)

    def write_bmp(path, img, bpp, top_down):
        h, w, _ = img.shape
        bpx = bpp // 8
        stride = (w * bpx + 3) & ~3
        rows = []
        for row in range(h):
            y = row if top_down else h - 1 - row
            px = img[y][:, ::-1]                                  # B, G, R
            if bpp == 32:
                px = np.concatenate([px, np.full((w, 1), 255, np.uint8)], 1)
            line = px.tobytes()
            rows.append(line + b"\0" * (stride - len(line)))
        data = b"".join(rows)
        hdr = b"BM" + struct.pack("<IHHI", 54 + len(data), 0, 0, 54)
        hdr += struct.pack("<IiiHHIIiiII", 40, w, -h if top_down else h, 1, bpp, 0, len(data), 2835, 2835, 0, 0)
        open(path, "wb").write(hdr + data)

    variants = {"a24.bmp": (24, False), "a32.bmp": (32, False), "a24td.bmp": (24, True)}
    for name, (bpp, td) in variants.items():
        write_bmp(tmp_path / name, rgb, bpp, td)
        assert np.array_equal(vrc.load_bmp(str(tmp_path / name)), rgb), name
    odd = np.arange(7 * 5 * 3, dtype=np.uint8).reshape(5, 7, 3)      # row padding: 7 * 3 = 21 -> 24 bytes
    write_bmp(tmp_path / "odd.bmp", odd, 24, False)
    assert np.array_equal(vrc.load_bmp(str(tmp_path / "odd.bmp")), odd)
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n#include <cstdio>\nint main(int c, char** v){ uint32_t w, h; auto p = vrc_host::loadBMP(v[1], &w, &h);'
           'std::fwrite(p.data(), 1, p.size(), stdout); std::fprintf(stderr, "%%u %%u", w, h); return 0; }\n') % hdr
    exe = str(tmp_path / "bmp_test")
    subprocess.run(["g++", "-std=c++14", "-x", "c++", "-", "-o", exe, "-L" + os.path.join(ROOT, "cpuvoxelraycaster_amd"),
                    "-l:libvrc_hip.so", "-Wl,-rpath," + os.path.join(ROOT, "cpuvoxelraycaster_amd"), "-Wl,-rpath,/opt/rocm/lib"],
                   input=src.encode(), check=True)
    for name in list(variants) + ["odd.bmp"]:
        out = subprocess.run([exe, str(tmp_path / name)], capture_output=True)
        want = odd if name == "odd.bmp" else rgb
        assert out.stderr.decode() == f"{want.shape[1]} {want.shape[0]}" and out.stdout == want.tobytes(), name
    ref = os.path.join(ROOT, "tests", "golden")                  # the reference's own res/grass_{top,side}_16x16.bmp, as data
    t, s = vrc.load_textures_bmp(os.path.join(ref, "grass_top_16x16.bmp"), os.path.join(ref, "grass_side_16x16.bmp"))
    assert np.array_equal(t, top) and np.array_equal(s, side)
    out = subprocess.run([exe, os.path.join(ref, "grass_side_16x16.bmp")], capture_output=True)
    assert out.stdout == side.tobytes()
