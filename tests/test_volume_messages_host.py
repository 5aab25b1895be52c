"""Every refusal of the vrc_volume_*, vrc_labels_* and vrc_distance_* entry points that is decided before the first HIP
call, on a machine without a GPU: the return code and the WHOLE vrc_last_error() text, as literals.  The handles are not
volumes, labels or fields at all -- a null handle where the null check is under test, otherwise a block of bytes that reads
as "depth 0 on device 0" -- so a call that reached the device would fail in another way, and nothing is written."""
import ctypes as C

import numpy as np
import pytest

HOST, DEVICE = 0, 1
TOO_MANY_VOXELS = 0x7FFFFFFF * 256 + 1
TOO_MANY_ITEMS = 0x80000000


def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


# zero: depth 0, device 0, count 0 whatever the layout; OTHER: a second one; ONES: every field differs from ZERO's;
# DEVICE_1: `device` is the first member of all three handle types; THREE_PIECES: vrc_labels::count is the 64-bit member at
# byte 8
ZERO, OTHER, ONES = handle(), handle(), handle(0x01010101)
DEVICE_1, THREE_PIECES = handle(w0=1), handle(w2=3)
U32 = np.zeros(16, np.uint32)
I32 = np.zeros(16, np.int32)
U64 = np.zeros(8, np.uint64)
OUT = C.c_void_p(0x55)


def affine(m=None, t=None, reserved=0):
    from cpuvoxelraycaster_amd import capi
    a = capi.Affine()
    for i, v in enumerate(m or [65536, 0, 0, 0, 65536, 0, 0, 0, 65536]):
        a.m[i] = v
    for i, v in enumerate(t or [0, 0, 0]):
        a.t[i] = v
    a.reserved = reserved
    return a


def p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.cast(a, C.c_void_p)


def list_in_cases(name, items, too_many, extra=()):
    """the calls  f(v, n, list, *extra, mem, stream)  with one list in: set_voxels, fill_boxes, fill_spheres, xor_mesh"""
    n_over = TOO_MANY_VOXELS if items == "voxels" else TOO_MANY_ITEMS
    return [(name, (None, 1, p(U32), *extra, HOST, None), "null volume"),
            (name, (p(ZERO), 1, p(U32), *extra, 2, None), "bad mem kind 2"),
            (name, (p(ZERO), 1, p(U32), *extra, -1, None), "bad mem kind -1"),
            (name, (p(ZERO), 1, None, *extra, HOST, None), "null buffer"),
            (name, (p(ZERO), n_over, p(U32), *extra, DEVICE, None), "too many %s for one launch" % too_many)]


def list_in_out_cases(name, null_handle, too_many=None):
    """the calls  f(h, n, list in, list out, mem, stream): get_voxels, count_boxes, labels_at, distance_at"""
    n_over = TOO_MANY_VOXELS if too_many == "voxels" else TOO_MANY_ITEMS
    return [(name, (None, 1, p(U32), p(U64), HOST, None), null_handle),
            (name, (p(ZERO), 1, p(U32), p(U64), 2, None), "bad mem kind 2"),
            (name, (p(ZERO), 1, p(U32), p(U64), -7, None), "bad mem kind -7"),
            (name, (p(ZERO), 1, None, p(U64), HOST, None), "null buffer"),
            (name, (p(ZERO), 1, p(U32), None, DEVICE, None), "null buffer"),
            (name, (p(ZERO), n_over, p(U32), p(U64), HOST, None), "too many %s for one launch" % too_many)]


def cases():
    out = []
    out += [("vrc_volume_create", (5, 0, None), "null argument"),
            ("vrc_volume_create", (1, 0, C.byref(OUT)), "depth 1 not in [2,10]"),
            ("vrc_volume_create", (11, 0, C.byref(OUT)), "depth 11 not in [2,10]"),
            ("vrc_volume_from_scene", (None, C.byref(OUT)), "null argument"),
            ("vrc_volume_from_scene", (p(ZERO), None), "null argument"),
            ("vrc_volume_from_scene", (p(ZERO), C.byref(OUT)), "depth 0 not in [2,10]"),
            ("vrc_volume_clone", (None, C.byref(OUT)), "null argument"),
            ("vrc_volume_clone", (p(ZERO), None), "null argument"),
            ("vrc_volume_commit", (None, C.byref(OUT), None), "null argument"),
            ("vrc_volume_commit", (p(ZERO), None, None), "null argument"),
            ("vrc_volume_download", (None, p(U32)), "null argument"),
            ("vrc_volume_download", (p(ZERO), None), "null argument"),
            ("vrc_volume_solid_count", (None, C.byref(C.c_uint64())), "null argument"),
            ("vrc_volume_solid_count", (p(ZERO), None), "null argument"),
            ("vrc_volume_edit_scratch_bytes", (None, C.byref(C.c_uint64())), "null argument"),
            ("vrc_volume_edit_scratch_bytes", (p(ZERO), None), "null argument")]
    out += list_in_cases("vrc_volume_set_voxels", "voxels", "voxels", (1,))
    out += list_in_cases("vrc_volume_fill_boxes", "items", "boxes", (1,))
    out += list_in_cases("vrc_volume_fill_spheres", "items", "spheres", (0,))
    out += list_in_cases("vrc_volume_xor_mesh", "items", "triangles")
    out += list_in_cases("vrc_volume_fill_spheres_at_hits", "items", "hits", (3, 1))
    out += [("vrc_volume_fill_spheres_at_hits", (p(ZERO), 1, p(U32), -1, 1, HOST, None), "radius -1 not in [0, 2^20]"),
            ("vrc_volume_fill_spheres_at_hits", (p(ZERO), 1, p(U32), (1 << 20) + 1, 0, DEVICE, None), "radius 1048577 not in [0, 2^20]")]
    out += list_in_out_cases("vrc_volume_get_voxels", "null volume", "voxels")
    out += list_in_out_cases("vrc_volume_count_boxes", "null volume", "boxes")

    name = "vrc_volume_copy_region"
    good = (p(U32), p(U32), p(I32))
    out += [(name, (None, p(OTHER), *good, 0, None), "null argument"),
            (name, (p(ZERO), None, *good, 0, None), "null argument"),
            (name, (p(ZERO), p(OTHER), None, p(U32), p(I32), 0, None), "null argument"),
            (name, (p(ZERO), p(OTHER), p(U32), None, p(I32), 0, None), "null argument"),
            (name, (p(ZERO), p(OTHER), p(U32), p(U32), None, 0, None), "null argument"),
            (name, (p(ZERO), p(ZERO), *good, 0, None), "source and destination are the same volume"),
            (name, (p(ZERO), p(OTHER), *good, 3, None), "bad op 3"),
            (name, (p(ZERO), p(OTHER), *good, -1, None), "bad op -1"),
            (name, (p(ZERO), p(ONES), *good, 1, None), "volumes on devices 16843009 and 0")]

    name = "vrc_volume_stamp_affine"
    ident = affine()
    box = (p(U32), p(U32))
    out += [(name, (None, p(OTHER), C.byref(ident), *box, 0, None), "null argument"),
            (name, (p(ZERO), None, C.byref(ident), *box, 0, None), "null argument"),
            (name, (p(ZERO), p(OTHER), None, *box, 0, None), "null argument"),
            (name, (p(ZERO), p(OTHER), C.byref(ident), None, p(U32), 0, None), "null argument"),
            (name, (p(ZERO), p(OTHER), C.byref(ident), p(U32), None, 0, None), "null argument"),
            (name, (p(ZERO), p(ZERO), C.byref(ident), *box, 0, None), "source and destination are the same volume"),
            (name, (p(ZERO), p(OTHER), C.byref(ident), *box, 26, None), "bad op 26"),
            (name, (p(ZERO), p(OTHER), C.byref(affine(reserved=1)), *box, 1, None), "reserved is 1, not 0"),
            (name, (p(ZERO), p(OTHER), C.byref(affine(m=[(1 << 20) + 1] + [0] * 8)), *box, 2, None), "m[0] = 1048577 beyond +-2^20"),
            (name, (p(ZERO), p(OTHER), C.byref(affine(m=[0] * 8 + [-(1 << 20) - 1])), *box, 2, None), "m[8] = -1048577 beyond +-2^20"),
            (name, (p(ZERO), p(OTHER), C.byref(affine(t=[(1 << 40) + 1, 0, 0])), *box, 0, None), "t[0] = 1099511627777 beyond +-2^40"),
            (name, (p(ZERO), p(OTHER), C.byref(affine(t=[0, 0, -(1 << 40) - 1])), *box, 0, None), "t[2] = -1099511627777 beyond +-2^40"),
            (name, (p(ZERO), p(ONES), C.byref(ident), *box, 0, None), "volumes on devices 16843009 and 0")]

    name = "vrc_volume_surface_count"
    out += [(name, (None, 1, p(U64)), "null volume"), (name, (p(ZERO), 1, None), "null counts")]
    name = "vrc_volume_extract_surface"
    out += [(name, (None, 1, 0, 0, 4, p(U32), None, HOST, None), "null volume"),
            (name, (p(ZERO), 1, 2, 0, 4, p(U32), None, HOST, None), "bad format 2"),
            (name, (p(ZERO), 1, 0, 0, 4, p(U32), None, 2, None), "bad mem kind 2"),
            (name, (p(ZERO), 1, 0, 0, 4, None, None, HOST, None), "null buffer with capacity 4"),
            (name, (p(ZERO), 1, 0, 0, 4, C.c_void_p(0x1004), None, DEVICE, None), "device buffer 0x1004 is not aligned to 16 bytes"),
            (name, (p(ZERO), 1, 1, 0, 4, C.c_void_p(0x1002), None, DEVICE, None), "device buffer 0x1002 is not aligned to 4 bytes")]

    name = "vrc_volume_flood"
    out += [(name, (None, p(OTHER), 6, 0, 0, None), "null volume"),
            (name, (p(ZERO), None, 6, 0, 0, None), "null volume"),
            (name, (p(ZERO), p(ZERO), 6, 0, 0, None), "region and medium are the same volume"),
            (name, (p(ZERO), p(OTHER), 18, 0, 0, None), "connectivity 18 is neither 6 nor 26"),
            (name, (p(ZERO), p(OTHER), 26, 2, 0, None), "bad through 2"),
            (name, (p(ZERO), p(ONES), 6, 1, 0, None), "volumes of depths 0 and 16843009"),
            (name, (p(ZERO), p(DEVICE_1), 6, 1, 0, None), "volumes on devices 0 and 1")]

    name = "vrc_volume_label_components"
    out += [(name, (None, 6, 0, C.byref(OUT), None), "null argument"),
            (name, (p(ZERO), 6, 0, None, None), "null argument"),
            (name, (p(ZERO), 0, 0, C.byref(OUT), None), "connectivity 0 is neither 6 nor 26"),
            (name, (p(ZERO), 26, -1, C.byref(OUT), None), "bad through -1")]
    name = "vrc_labels_components"
    out += [(name, (None, 0, 5, p(U32), HOST, None), "null labels"),
            (name, (p(ZERO), 0, 5, p(U32), 2, None), "bad mem kind 2"),
            (name, (p(ZERO), 0, 5, None, HOST, None), "null buffer with capacity 5")]
    out += list_in_out_cases("vrc_labels_at", "null labels", "voxels")
    name = "vrc_labels_select"
    keep = p(U32)
    out += [(name, (None, keep, p(OTHER), 0, HOST, None), "null argument"),
            (name, (p(ZERO), keep, None, 0, HOST, None), "null argument"),
            (name, (p(ZERO), keep, p(OTHER), 3, HOST, None), "bad op 3"),
            (name, (p(ZERO), keep, p(OTHER), 0, 2, None), "bad mem kind 2"),
            (name, (p(ZERO), keep, p(ONES), 1, DEVICE, None), "labels of depth 0, volume of depth 16843009"),
            (name, (p(ZERO), keep, p(DEVICE_1), 1, DEVICE, None), "labels on device 0, volume on device 1"),
            (name, (p(THREE_PIECES), None, p(OTHER), 2, HOST, None), "null keep with 3 components")]

    name = "vrc_volume_distance_field"
    out += [(name, (None, 0, 0, C.byref(OUT), None), "null argument"),
            (name, (p(ZERO), 0, 0, None, None), "null argument"),
            (name, (p(ZERO), 2, 0, C.byref(OUT), None), "bad to 2"),
            (name, (p(ZERO), 1, 1, C.byref(OUT), None), "depth 0 not in [2,10]")]
    out += list_in_out_cases("vrc_distance_at", "null distance field", "voxels")
    name = "vrc_distance_download"
    out += [(name, (None, p(U32)), "null argument"), (name, (p(ZERO), None), "null argument")]
    name = "vrc_distance_select"
    out += [(name, (None, 0, 1, p(OTHER), 0, None), "null argument"),
            (name, (p(ZERO), 0, 1, None, 0, None), "null argument"),
            (name, (p(ZERO), 0, 1, p(OTHER), -1, None), "bad op -1"),
            (name, (p(ZERO), 5, 4, p(OTHER), 1, None), "lo 5 above hi 4"),
            (name, (p(ZERO), 0, 4, p(ONES), 2, None), "field of depth 0, volume of depth 16843009"),
            (name, (p(ZERO), 0, 4, p(DEVICE_1), 2, None), "field on device 0, volume on device 1")]

    # two refusals at once: the one that wins (at the end, so that the cases above keep their numbers)
    name = "vrc_volume_copy_region"
    out += [(name, (p(ZERO), p(ZERO), *good, 3, None), "source and destination are the same volume"),
            (name, (p(ZERO), p(ONES), *good, 3, None), "bad op 3"),
            (name, (p(DEVICE_1), p(ZERO), *good, -1, None), "bad op -1"),
            (name, (p(DEVICE_1), p(ZERO), *good, 2, None), "volumes on devices 0 and 1")]
    name = "vrc_volume_stamp_affine"
    out += [(name, (p(ZERO), p(ZERO), C.byref(ident), *box, 3, None), "source and destination are the same volume"),
            (name, (p(ZERO), p(ZERO), C.byref(affine(reserved=1)), *box, 0, None), "source and destination are the same volume"),
            (name, (p(ZERO), p(ONES), C.byref(ident), *box, 3, None), "bad op 3"),
            (name, (p(ZERO), p(OTHER), C.byref(affine(reserved=1)), *box, 3, None), "bad op 3"),
            (name, (p(DEVICE_1), p(ZERO), C.byref(affine(reserved=2)), *box, 0, None), "reserved is 2, not 0"),
            (name, (p(DEVICE_1), p(ZERO), C.byref(ident), *box, 2, None), "volumes on devices 0 and 1")]
    name = "vrc_volume_flood"
    out += [(name, (p(ZERO), p(ZERO), 18, 0, 0, None), "region and medium are the same volume"),
            (name, (p(ZERO), p(ONES), 18, 0, 0, None), "connectivity 18 is neither 6 nor 26"),
            (name, (p(ZERO), p(DEVICE_1), 6, 2, 0, None), "bad through 2"),
            (name, (p(ONES), p(DEVICE_1), 26, 0, 0, None), "volumes of depths 16843009 and 0"),
            (name, (p(DEVICE_1), p(ZERO), 26, 0, 0, None), "volumes on devices 1 and 0")]
    return out


CASES = cases()


@pytest.mark.parametrize("index", range(len(CASES)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    name, args, text = CASES[index]
    assert getattr(L, name)(*args) == -1                                     # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
    # nothing was written through any handle or buffer
    assert not any(ZERO) and not any(OTHER) and all(v == 0x01010101 for v in ONES)
    assert list(DEVICE_1) == [1] + [0] * 127 and list(THREE_PIECES) == [0, 0, 3] + [0] * 125
    assert not U32.any() and not I32.any() and not U64.any() and OUT.value == 0x55


def test_every_entry_point_is_in_the_table():
    from cpuvoxelraycaster_amd import capi
    listed = {c[0] for c in CASES}
    # these refuse nothing: a null handle is 0 / a no-op
    silent = {"vrc_volume_destroy", "vrc_volume_depth", "vrc_labels_destroy", "vrc_labels_count", "vrc_labels_depth", "vrc_labels_bytes",
              "vrc_distance_destroy", "vrc_distance_depth", "vrc_distance_bytes", "vrc_distance_data"}
    names = {n for n in capi.SYMBOLS if n.startswith(("vrc_volume_", "vrc_labels_", "vrc_distance_"))}
    assert names == listed | silent and not listed & silent
