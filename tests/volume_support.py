"""What the voxel-volume tests share: uploading a numpy occupancy array, a test stream, the record helpers of the posed-piece
tests, the committed / expected LNode[] of a volume, and the g++ lines of the C++ drivers and header checks.  One copy; a new
feature's tests import these names.  The library is imported inside the functions, so collecting needs no built library."""
import ctypes as C
import os
import subprocess

import numpy as np

import contact_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cpuvoxelraycaster_amd")


# ---- volumes and labels ------------------------------------------------------------------------------------------

def volume_of(vol, depth=None):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume(int(vol.shape[0]).bit_length() - 1 if depth is None else depth)
    if vol.any():
        volume.setVoxels(np.argwhere(vol))
    return volume


def labels_of(vol, connectivity=6, through_empty=False):
    medium = volume_of(vol)
    labels = medium.labelComponents(connectivity, through_empty)
    medium.close()
    return labels


def all_coordinates(S):
    """(S^3 + 6, 3): every voxel in [x, y, z] order, then six coordinates outside the volume"""
    inside = np.indices((S, S, S)).reshape(3, -1).T
    outside = [[S, 0, 0], [0, S, 0], [0, 0, S], [S + 7, S, S], [0xFFFFFFFF, 0, 0], [1, 0x80000000, 1]]
    return np.concatenate([inside, np.array(outside, np.int64)]).astype(np.uint32)


class Stream:
    def __enter__(self):
        import cpuvoxelraycaster_amd as vrc
        self.L = vrc.capi.load()
        self.h = C.c_void_p()
        vrc.capi.check(self.L.vrc_stream_create(0, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        self.L.vrc_stream_synchronize(0, self.h)
        self.L.vrc_stream_destroy(0, self.h)


# ---- a stream kept busy, so that what is enqueued behind it is late ------------------------------------------------

def device_words(a):
    """a numpy array of 32-bit items as an int32 tensor in device memory"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


# How many times the ballast fills its 512^3 volume.  Sized on the MI355X so that the ballast lasts at least four times the
# longest host-side enqueue of any call of test_gpu_volume_ordering.py (its docstring and docs/NOTEBOOK.md have the figures).
BALLAST_FILLS = 2048


class Ballast:
    """One 512^3 volume and BALLAST_FILLS whole-volume device-memory fills of it: enqueue(stream) keeps the stream busy
    for milliseconds, so that the next call enqueued on it lands late -- an edit to lose a race against.  The fills are
    the items of ONE vrc_volume_fill_boxes list, so that the backlog stands as soon as the call returns, however slow the
    host is at enqueuing; a second call clears the volume again."""

    def __init__(self, fills=BALLAST_FILLS):
        import cpuvoxelraycaster_amd as vrc
        self.big, self.fills = vrc.VoxelVolume(9), fills
        self.whole = device_words(np.tile(np.array([[0, 0, 0, 512, 512, 512]], np.uint32), (fills, 1)))

    def enqueue(self, stream):
        self.big.fillBoxesDevice(self.fills - 1, self.whole.data_ptr(), True, stream)
        self.big.fillBoxesDevice(1, self.whole.data_ptr(), False, stream)

    def close(self):
        self.big.close()


def event_on(stream):
    """a torch event recorded on a vrc_stream_create stream right now: event.query() is False while the work enqueued on
    the stream so far is still running"""
    import torch
    event = torch.cuda.Event()
    event.record(torch.cuda.ExternalStream(stream.value))
    return event


# ---- records of posed pieces -------------------------------------------------------------------------------------

def affine_records(maps):
    import cpuvoxelraycaster_amd as vrc
    out = np.zeros(len(maps), vrc.capi.AFFINE_DTYPE)
    for i, (m, t) in enumerate(maps):
        out[i] = (m, 0, t)
    return out


def tuples(records):
    return [contact_model.record_tuple(r) for r in records]


def differing(got, want):
    """the first few records that differ, for the assertion's message"""
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]


# ---- committed scenes --------------------------------------------------------------------------------------------

def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def terrain_volume(heights, depth):
    """main.cpp:65-74 as dense occupancy [x, y, z]: column (x, z) solid for y in [S/2 + 1, S/2 + lim)"""
    S = 1 << depth
    lim = np.maximum(16, np.minimum(S, heights[:S, :S].astype(np.int64)))
    y = np.arange(S)[None, :, None]
    return ((y >= S // 2 + 1) & (y < S // 2 + lim[:, None, :])).astype(np.uint8)


def expected_nodes(vol, depth):
    import cpuvoxelraycaster_amd as vrc
    import oracle_lib as O
    if depth <= 5:
        return O.compile_voxels(depth, np.argwhere(vol))
    return vrc.build_volume_lsvo(vol, depth)


def committed(volume, timed=False):
    """the LNode[] the volume commits; timed: the commit must also report a build time"""
    svo = volume.commit()
    nodes = svo.downloadNodes()
    if timed:
        assert svo.build_ms is not None and svo.build_ms > 0
    svo.close()
    return nodes


def fnv1a(buf):
    h = 1469598103934665603
    for b in bytes(buf):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- the C++ side ------------------------------------------------------------------------------------------------

def compile_cpp_main(outdir, name, flags=("-Wall",), libs=()):
    """tests/cpp/<name>.cpp linked against the built library, as outdir/<name>; flags go before the source, libs after the
    library"""
    exe = str(outdir / name)
    subprocess.check_call(["g++", "-std=c++14", "-O1", *flags, os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           "-o", exe, "-L" + PKG, "-l:libvrc_hip.so", *libs, "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_program(exe, *args, timeout=120):
    """the completed run of a program that must succeed; what it printed is printed"""
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout.strip())
    return out


def run_cpp_main(tmp_path, name, *args, timeout=120, flags=("-Wall",), libs=()):
    return run_program(compile_cpp_main(tmp_path, name, flags, libs), *args, timeout=timeout)


def check_cpp_syntax(src_or_path, strict=False):
    """g++ -fsyntax-only over a source text (anything with a newline in it) or a file; strict: -Wall -Werror"""
    cmd = ["g++", "-std=c++14"] + (["-Wall", "-Werror"] if strict else []) + ["-fsyntax-only"]
    if "\n" in src_or_path:
        subprocess.run(cmd + ["-x", "c++", "-"], input=src_or_path.encode(), check=True)
    else:
        subprocess.run(cmd + [src_or_path], check=True)
