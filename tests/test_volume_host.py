"""The editable volume's host side, on a machine without a GPU: vrc_hit_to_voxel against the oracle's own hits,
the argument checks of the vrc_volume_* / vrc_renderer_set_scene entry points that need no device, and the C++ host
adapter with HipVoxelVolume / HipRayCaster::setScene under a plain C++14 compiler."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 20000
MIN_UNIT_HITS = 300


def _hit_to_voxel(L, depth, rec):
    from cpuvoxelraycaster_amd import capi
    voxel, neighbour, has = np.full(3, 0xdeadbeef, np.uint32), np.full(3, 0xdeadbeef, np.uint32), C.c_int(-1)
    one = np.zeros(1, capi.HIT_DTYPE)
    one[0] = rec
    rc = L.vrc_hit_to_voxel(depth, capi.ptr(one), capi.ptr(voxel), capi.ptr(neighbour), C.byref(has))
    return rc, voxel.astype(np.int64), neighbour.astype(np.int64), has.value


@pytest.mark.parametrize("depth", [3, 5, 7])
def test_hit_to_voxel_matches_oracle(built, depth):
    """Random 8 % volumes, 20 000 random rays with origins in [0, 3)^3 cast by the oracle: every unit-voxel hit maps
    to a solid voxel; a single-axis normal whose neighbour lies inside names an EMPTY neighbour; zero normals and
    neighbours outside the volume report has_neighbour == 0; a miss is VRC_ERR_INVALID."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    S = 1 << depth
    rng = np.random.default_rng(1000 + depth)
    vol = rng.random((S, S, S)) < 0.08
    nodes = O.compile_voxels(depth, np.argwhere(vol))
    org = (rng.random((N_RAYS, 3)) * 3.0).astype(np.float32)
    dir_ = rng.standard_normal((N_RAYS, 3)).astype(np.float32)
    dir_ /= np.linalg.norm(dir_, axis=1, keepdims=True)
    hits = O.cast_rays(nodes, depth, org, dir_, threads=4)
    assert hits.dtype.itemsize == capi.HIT_DTYPE.itemsize
    unit = misses = with_neighbour = zero_normal = outside = 0
    for h in hits:
        kind = int(h["hit"]) & 0xff
        rc, voxel, neighbour, has = _hit_to_voxel(L, depth, h)
        if kind != 1:
            assert rc == -1 and kind == 0          # coef / bias 0: no LOD cut-offs among these rays
            misses += 1
            continue
        unit += 1
        assert rc == 0
        assert np.all(voxel >= 0) and np.all(voxel < S)
        assert vol[tuple(voxel)], (h, voxel)
        nz = np.flatnonzero(h["normal"])
        if len(nz) == 1:
            want = voxel.copy()
            want[nz[0]] -= int(np.sign(h["normal"][nz[0]]))
            if np.all(want >= 0) and np.all(want < S):
                assert has == 1 and np.array_equal(neighbour, want)
                assert not vol[tuple(neighbour)], (h, voxel, neighbour)
                with_neighbour += 1
            else:
                assert has == 0
                outside += 1
        else:
            assert len(nz) == 0 and has == 0       # the ray started inside a solid voxel
            zero_normal += 1
    print(f"depth {depth}: {unit} unit-voxel hits, {with_neighbour} with an empty neighbour, {outside} at the volume's face, "
          f"{zero_normal} zero normals, {misses} misses")
    assert unit >= MIN_UNIT_HITS and with_neighbour > 0 and misses > 0


def test_hit_to_voxel_arguments(built):
    from cpuvoxelraycaster_amd import capi
    import cpuvoxelraycaster_amd as vrc
    L = capi.load()
    rec = np.zeros(1, capi.HIT_DTYPE)
    rec["hit"] = 1
    rec["position"] = (1.5, 1.25, 1.999)
    rec["normal"] = (0, -2, 0)
    v, n, has = np.zeros(3, np.uint32), np.zeros(3, np.uint32), C.c_int()
    assert L.vrc_hit_to_voxel(3, capi.ptr(rec), capi.ptr(v), capi.ptr(n), C.byref(has)) == 0
    assert list(v) == [3, 5, 0] and list(n) == [3, 6, 0] and has.value == 1
    assert L.vrc_hit_to_voxel(3, capi.ptr(rec), capi.ptr(v), None, None) == 0          # neighbour is optional
    assert vrc.hit_to_voxel(3, rec[0]) == ((3, 5, 0), (3, 6, 0))
    rec["normal"] = (0, 0, 4)                                                           # neighbour z = -1: outside
    assert vrc.hit_to_voxel(3, rec[0]) == ((3, 5, 0), None)
    assert L.vrc_hit_to_voxel(1, capi.ptr(rec), capi.ptr(v), capi.ptr(n), C.byref(has)) == -1
    assert L.vrc_hit_to_voxel(12, capi.ptr(rec), capi.ptr(v), capi.ptr(n), C.byref(has)) == -1
    assert L.vrc_hit_to_voxel(3, None, capi.ptr(v), capi.ptr(n), C.byref(has)) == -1
    assert L.vrc_hit_to_voxel(3, capi.ptr(rec), None, capi.ptr(n), C.byref(has)) == -1
    rec["hit"] = 2 | (3 << 8)                                                           # LOD cut-off
    assert L.vrc_hit_to_voxel(3, capi.ptr(rec), capi.ptr(v), capi.ptr(n), C.byref(has)) == -1
    rec["hit"] = 0
    with pytest.raises(vrc.VrcError):
        vrc.hit_to_voxel(3, rec[0])
    rec["hit"] = 1
    rec["position"] = (2.5, 1.25, 1.5)                                                  # not a position of the walk
    assert L.vrc_hit_to_voxel(3, capi.ptr(rec), capi.ptr(v), capi.ptr(n), C.byref(has)) == -1


def test_volume_argument_validation_needs_no_gpu(built):
    """Bad arguments are refused before any HIP call; without a device creation fails loudly."""
    import torch
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    h = C.c_void_p()
    for depth in (0, 1, 11, 12):
        assert L.vrc_volume_create(depth, 0, C.byref(h)) == -1, depth
        assert b"[2,10]" in L.vrc_last_error()
    assert L.vrc_volume_create(5, 0, None) == -1
    assert L.vrc_volume_from_scene(None, C.byref(h)) == -1
    xyz = np.zeros((4, 3), np.uint32)
    assert L.vrc_volume_set_voxels(None, 4, capi.ptr(xyz), 1, 0, None) == -1
    assert L.vrc_volume_fill_boxes(None, 1, capi.ptr(xyz), 1, 0, None) == -1
    assert L.vrc_volume_commit(None, C.byref(h), None) == -1
    assert L.vrc_volume_download(None, capi.ptr(xyz)) == -1
    n = C.c_uint64()
    assert L.vrc_volume_solid_count(None, C.byref(n)) == -1
    assert L.vrc_volume_depth(None) == 0 and L.vrc_volume_destroy(None) == 0
    assert L.vrc_renderer_set_scene(None, None) == -1
    assert b"vrc_renderer_set_scene" in L.vrc_last_error()
    if not torch.cuda.is_available():
        assert L.vrc_volume_create(5, 0, C.byref(h)) == -2        # VRC_ERR_NO_DEVICE: no CPU fallback


def test_host_adapter_with_volume_classes_compiles(built):
    """HipVoxelVolume / HipRayCaster::setScene in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'void use(vrc_host::HipRayCaster& rc, const vrc_host::HipLSVO& svo) {\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> vol = vrc_host::HipVoxelVolume::fromScene(svo);\n'
           '    vrc_host::HipVoxelVolume empty(5);\n'
           '    vol->setCell(vrc_host::Cell::Empty, vrc_host::Cell::None, 1, 2, 3);\n'
           '    vol->setCell(vrc_host::Cell::Solid, vrc_host::Cell::Grass, 1, 2, 4);\n'
           '    vol->fillBox(0, 0, 0, 4, 4, 4, false);\n'
           '    float ms = 0;\n'
           '    std::unique_ptr<vrc_host::HipLSVO> next = vol->commit(&ms);\n'
           '    rc.setScene(*next);\n'
           '    (void)vol->solidCount(); (void)vol->depth();\n'
           '}\nint main(){ return 0; }\n') % hdr
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], input=src.encode(), check=True)
    main = os.path.join(ROOT, "tests", "cpp", "voxel_volume_main.cpp")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", main], check=True)
