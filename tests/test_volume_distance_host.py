"""The distance field on a machine without a GPU: the refusals that need no device, the stats record's size, the C++ host
adapter with HipVoxelDistance under a plain C++14 compiler, and the yardstick of the GPU tests itself -- the numpy model
of tests/distance_model.py against the definition taken literally (a brute-force minimum over all feature voxels plus the
wall term)."""
import ctypes as C
import os

import numpy as np
import pytest

import distance_model as model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(vol, to_empty, outside):
    """D(p) = min over q in F of |p - q|^2, then the wall term, voxel by feature voxel"""
    S = vol.shape[0]
    F = np.argwhere((vol == 0) if to_empty else (vol != 0)).astype(np.int64)
    P = np.indices((S, S, S)).reshape(3, -1).T.astype(np.int64)
    big = np.int64(1) << 40
    D = np.full(len(P), big, np.int64)
    for q in F:
        D = np.minimum(D, ((P - q) ** 2).sum(axis=1))
    if outside:
        for a in range(3):
            D = np.minimum(D, np.minimum((P[:, a] + 1) ** 2, (S - P[:, a]) ** 2))
    return np.where(D >= big, model.NONE, D).astype(np.uint32).reshape(S, S, S)


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("to_empty", [False, True])
@pytest.mark.parametrize("S", [4, 8, 16])
def test_model_against_the_definition(S, to_empty, outside):
    rng = np.random.default_rng(1200 + S + 2 * int(to_empty) + int(outside))
    volumes = [(rng.random((S, S, S)) < density).astype(np.uint8) for density in (0.002, 0.05, 0.5, 0.95)]
    volumes += [np.zeros((S, S, S), np.uint8), np.ones((S, S, S), np.uint8)]
    for vol in volumes:
        D = model.field(vol, to_empty, outside)
        want = brute_force(vol, to_empty, outside)
        assert D.dtype == np.uint32 and np.array_equal(D, want), (S, to_empty, outside, int(vol.sum()))
        F = model.feature_set(vol, to_empty)
        assert (D[F] == 0).all()
        if not F.any() and not outside:
            assert (D == model.NONE).all()
        else:
            assert int(D.max()) <= 3 * (S - 1) ** 2
        m, arg = model.stats(D)
        finite = want[want != model.NONE]
        assert m == (int(finite.max()) if len(finite) else 0)
        if len(finite):
            assert want[arg] == m and not (want.reshape(-1)[:(arg[0] * S + arg[1]) * S + arg[2]] == m).any()
        else:
            assert arg == (0, 0, 0)


def test_model_select_and_tools():
    S = 8
    vol = np.zeros((S, S, S), np.uint8)
    vol[4, 4, 4] = 1
    D = model.field(vol)
    assert int(model.select(D, 0, 0).sum()) == 1 and int(model.select(D, 1, 1).sum()) == 6
    assert int(model.select(D, 0, model.NONE).sum()) == S ** 3
    assert int(model.dilate(vol, 1).sum()) == 7 and np.array_equal(model.dilate(vol, 0), vol != 0)
    assert int(model.erode(model.dilate(vol, 1), 1).sum()) == 1
    box = np.zeros((S, S, S), np.uint8)
    box[0:4, 2:6, 2:6] = 1
    assert int(model.erode(box, 1).sum()) == 3 * 2 * 2            # the face x = 0 is a wall
    assert int(model.erode(box, 1, True).sum()) == 2 * 2 * 2      # ... unless the border is open
    assert int(model.hollow(box, 0).sum()) == 0 and int(model.hollow(box, 1).sum()) == 64 - 3 * 2 * 2
    assert (model.field(np.zeros((S, S, S), np.uint8), False, True) == model.wall_term(S)).all()


def test_distance_stats_layout(built):
    from cpuvoxelraycaster_amd import capi
    assert C.sizeof(capi.DistanceStats) == 32
    assert [getattr(capi.DistanceStats, f).offset for f in ("features", "max_d2", "argmax", "reserved")] == [0, 8, 12, 24]
    assert capi.VRC_DISTANCE_NONE == model.NONE == 0xFFFFFFFF
    hdr = os.path.join(ROOT, "include", "vrc.h")
    src = '#include "%s"\nstatic_assert(sizeof(vrc_distance_stats) == 32, "vrc_distance_stats");\nint main() { return 0; }\n' % hdr
    check_cpp_syntax(src)


def test_distance_refusals_need_no_gpu(built):
    """NULL handles, a `to` other than 0 / 1, an unknown op, lo > hi, a bad mem kind and a field against a volume of
    another depth are VRC_ERR_INVALID with the function's name before any HIP call: the handles here are not volumes or
    fields at all, and nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b = (C.c_uint32 * 128)(), (C.c_uint32 * 128)()        # 512 zero bytes each: "depth 0 on device 0" whatever the layout
    pa, pb = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    out, stats = C.c_void_p(0x55), capi.DistanceStats()
    stats.max_d2 = 7
    for medium, to, o in [(None, 0, C.byref(out)), (None, 1, C.byref(out)), (pa, 0, None), (pa, 2, C.byref(out)), (pa, -1, C.byref(out)),
                          (pa, 6, C.byref(out))]:
        for outside in (0, 1):
            for st in (None, C.byref(stats)):
                assert L.vrc_volume_distance_field(medium, to, outside, o, st) == -1, (to, outside)
                assert L.vrc_last_error().startswith(b"vrc_volume_distance_field"), L.vrc_last_error()
    assert out.value == 0x55 and stats.max_d2 == 7 and stats.features == 0

    assert L.vrc_distance_destroy(None) == 0
    assert L.vrc_distance_depth(None) == 0 and L.vrc_distance_bytes(None) == 0 and not L.vrc_distance_data(None)
    xyz, d2 = np.zeros(3, np.uint32), np.full(1, 9, np.uint32)
    host = np.full(4, 9, np.uint32)
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_distance_at(None, 1, capi.ptr(xyz), capi.ptr(d2), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_distance_at")
    for mem in (-1, 2, 7):
        assert L.vrc_distance_at(pa, 1, capi.ptr(xyz), capi.ptr(d2), mem, None) == -1
        assert b"bad mem kind" in L.vrc_last_error()
    assert L.vrc_distance_at(pa, 1, None, capi.ptr(d2), capi.VRC_MEM_HOST, None) == -1
    assert L.vrc_distance_at(pa, 1, capi.ptr(xyz), None, capi.VRC_MEM_HOST, None) == -1
    assert L.vrc_distance_download(None, capi.ptr(host)) == -1 and L.vrc_distance_download(pa, None) == -1
    assert L.vrc_last_error().startswith(b"vrc_distance_download")
    assert L.vrc_distance_select(None, 0, 1, pb, capi.VRC_COPY_REPLACE, None) == -1
    assert L.vrc_distance_select(pa, 0, 1, None, capi.VRC_COPY_REPLACE, None) == -1
    assert L.vrc_last_error().startswith(b"vrc_distance_select")
    for op in (-1, 3, 26):
        assert L.vrc_distance_select(pa, 0, 1, pb, op, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_distance_select: bad op"), L.vrc_last_error()
    for lo, hi in [(1, 0), (0xFFFFFFFF, 0xFFFFFFFE), (5, 4)]:
        assert L.vrc_distance_select(pa, lo, hi, pb, capi.VRC_COPY_OR, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_distance_select: lo"), L.vrc_last_error()
    # a volume whose every field differs from the field's: a depth (or device) mismatch
    for i in range(128):
        b[i] = 0x01010101
    for op in (capi.VRC_COPY_REPLACE, capi.VRC_COPY_OR, capi.VRC_COPY_ANDNOT):
        assert L.vrc_distance_select(pa, 0, 0xFFFFFFFF, pb, op, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_distance_select: field"), L.vrc_last_error()
    assert not any(a) and all(v == 0x01010101 for v in b)
    assert d2[0] == 9 and (host == 9).all()


def test_negative_radius_is_refused_before_any_device_call(built):
    """VoxelVolume.dilate / erode / openShape / closeShape / hollow with a negative value raise ValueError without touching
    the handle (there is none here)."""
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume.__new__(vrc.VoxelVolume)
    volume._h, volume.depth, volume.device = None, 5, 0
    for tool in (volume.dilate, volume.erode, volume.openShape, volume.closeShape, volume.hollow):
        with pytest.raises(ValueError):
            tool(-1)


def test_host_adapter_with_distance_compiles(built):
    """HipVoxelDistance and HipVoxelVolume::distanceField / dilate / erode / hollow in the header-only adapter: C++14, no
    GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world) {\n'
           '    vrc_host::HipVoxelDistance field = world.distanceField(true, false);\n'
           '    const vrc_distance_stats& stats = field.stats();\n'
           '    vrc_host::HipVoxelVolume shell(world.depth());\n'
           '    field.select(1, 4, shell, VRC_COPY_REPLACE);\n'
           '    const uint32_t xyz[3] = {1, 2, 3};\n'
           '    std::vector<uint32_t> d2 = field.at(xyz, 1);\n'
           '    std::vector<uint32_t> all = field.download();\n'
           '    world.dilate(2); world.erode(2, true); world.hollow(1);\n'
           '    return stats.features + stats.max_d2 + d2[0] + all.size() + field.bytes() + field.depth() + (field.data() != nullptr);\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
