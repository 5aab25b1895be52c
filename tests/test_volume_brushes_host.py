"""The brush / copy / query entry points of the editable volume on a machine without a GPU: what can be refused without a
volume is refused with VRC_ERR_INVALID before any HIP call, and the C++ host adapter with the new HipVoxelVolume members
compiles under a plain C++14 compiler."""
import ctypes as C
import os

import numpy as np

from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brush_argument_validation_needs_no_gpu(built):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    p = capi.ptr
    buf = np.zeros(64, np.uint32)
    hits = np.zeros(2, capi.HIT_DTYPE)
    out8, out64 = np.zeros(8, np.uint8), np.zeros(8, np.uint64)
    lo, size, dst_lo = np.zeros(3, np.uint32), np.ones(3, np.uint32), np.zeros(3, np.int32)
    h = C.c_void_p()
    for mem in (0, 1):
        for n in (0, 2):
            assert L.vrc_volume_fill_spheres(None, n, p(buf), 1, mem, None) == -1
            assert b"vrc_volume_fill_spheres: null volume" in L.vrc_last_error()
            assert L.vrc_volume_fill_spheres_at_hits(None, n, p(hits), 1, 0, mem, None) == -1
            assert b"vrc_volume_fill_spheres_at_hits" in L.vrc_last_error()
            assert L.vrc_volume_get_voxels(None, n, p(buf), p(out8), mem, None) == -1
            assert b"vrc_volume_get_voxels" in L.vrc_last_error()
            assert L.vrc_volume_count_boxes(None, n, p(buf), p(out64), mem, None) == -1
            assert b"vrc_volume_count_boxes" in L.vrc_last_error()
    for op in (0, 1, 2, 3):
        assert L.vrc_volume_copy_region(None, None, p(lo), p(size), p(dst_lo), op, None) == -1
        assert b"vrc_volume_copy_region" in L.vrc_last_error()
    assert L.vrc_volume_clone(None, C.byref(h)) == -1
    assert L.vrc_volume_clone(None, None) == -1
    assert b"vrc_volume_clone" in L.vrc_last_error()
    assert (capi.VRC_COPY_REPLACE, capi.VRC_COPY_OR, capi.VRC_COPY_ANDNOT) == (0, 1, 2)


def test_null_out_of_clone_is_refused_before_the_volume_is_read(built):
    """out == NULL with a volume pointer that is not one: the call must not touch it"""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    not_a_volume = np.zeros(64, np.uint8)
    assert L.vrc_volume_clone(capi.ptr(not_a_volume), None) == -1
    assert not not_a_volume.any()


def test_host_adapter_with_brush_members_compiles(built):
    """the new HipVoxelVolume members in the header-only adapter: C++14, no GLM, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'void use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& clipboard, const vrc_host::HipLSVO& svo) {\n'
           '    std::vector<vrc_host::Vec3> org(4), dir(4);\n'
           '    const std::vector<vrc_hit> hits = svo.castRaysRecords(org, dir);\n'
           '    world.fillSpheresAtHits(hits, 3, false);\n'
           '    world.fillSpheresAtHitsDevice(0, nullptr, 3, true, nullptr);\n'
           '    world.fillSpheres({{1, 2, 3, 4}, {-5, 6, 7, 0}}, true);\n'
           '    world.fillSpheresDevice(0, nullptr, false);\n'
           '    const uint32_t lo[3] = {0, 0, 0}, size[3] = {32, 32, 32};\n'
           '    const int32_t at[3] = {-3, 100, 7};\n'
           '    world.copyRegion(clipboard, lo, size, at, VRC_COPY_OR);\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> undo = world.clone();\n'
           '    std::vector<uint8_t> solid = undo->getVoxels({1, 2, 3});\n'
           '    std::vector<uint64_t> counts = undo->countBoxes({0, 0, 0, 8, 8, 8});\n'
           '    (void)solid; (void)counts;\n'
           '}\nint main(){ return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
    main = os.path.join(ROOT, "tests", "cpp", "voxel_brushes_main.cpp")
    check_cpp_syntax(main, strict=True)
