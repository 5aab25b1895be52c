"""ctypes binding of libvrc_hip.so (the C ABI of include/vrc.h).

Plumbing only: every compute call goes to the hand-written HIP kernels.  There
is no CPU fallback -- if the library is missing, or no HIP device is present,
calls raise VrcError."""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libvrc_hip.so")

VRC_MEM_HOST, VRC_MEM_DEVICE = 0, 1
VRC_COPY_REPLACE, VRC_COPY_OR, VRC_COPY_ANDNOT = 0, 1, 2
VRC_CONNECT_FACES, VRC_CONNECT_ALL = 6, 26
VRC_CELLS_FACES, VRC_CELLS_ALL = 6, 26
VRC_FLOOD_SOLID, VRC_FLOOD_EMPTY = 0, 1
VRC_COLUMNS_SOLID, VRC_COLUMNS_EMPTY = 1, 2
VRC_COLUMN_NONE = 0xffffffff
VRC_MORPH_DILATE, VRC_MORPH_ERODE = 0, 1
VRC_MORPH_SOLID, VRC_MORPH_EMPTY = 1, 2
VRC_MORPH_REACH = 16
VRC_MORPH_MAX_OFFSETS = 1 << 20
VRC_NO_COMPONENT = 0xffffffff
VRC_DISTANCE_NONE = 0xffffffff
VRC_SIGHT_THIN, VRC_SIGHT_TOUCH, VRC_SIGHT_PLAIN = 0, 1, 2
VRC_SIGHT_CLEAR, VRC_SIGHT_BLOCKED, VRC_SIGHT_OUTSIDE = 0, 1, 2
VRC_STROKE_LIMIT = 8192
VRC_MESH_FRAC_BITS = 6
VRC_RASTER_TOUCHED, VRC_RASTER_THIN = 0, 1
VRC_AFFINE_FRAC_BITS = 16
VRC_FACE_XN, VRC_FACE_XP, VRC_FACE_YN, VRC_FACE_YP, VRC_FACE_ZN, VRC_FACE_ZP = range(6)
VRC_SURFACE_FACES, VRC_SURFACE_TRIANGLES = 0, 1
VRC_VOXELS_ALL, VRC_VOXELS_SURFACE, VRC_VOXELS_INTERIOR = 0, 1, 2
VRC_VOXELS_XYZ, VRC_VOXELS_NEIGHBOURS = 0, 1

HIT_DTYPE = np.dtype([
    ("position", "<f4", 3), ("normal", "<f4", 3), ("voxel_coord", "<f4", 2),
    ("hit", "<u4"), ("node", "<u4"), ("distance", "<f4"), ("complexity", "<u4"),
])
LNODE_DTYPE = np.dtype([("color", "u1"), ("child_mask", "u1"), ("leaf_mask", "u1"),
                        ("pad", "u1"), ("child_offset", "<u4")])
assert HIT_DTYPE.itemsize == 48 and LNODE_DTYPE.itemsize == 8
# vrc_component (include/vrc.h): one record per connected component
COMPONENT_DTYPE = np.dtype([("first", "<u4", 3), ("lo", "<u4", 3), ("hi", "<u4", 3), ("reserved", "<u4"), ("voxels", "<u8")])
assert COMPONENT_DTYPE.itemsize == 48
# vrc_piece_moments (include/vrc.h): n, the sums of c and of the six products c_a c_b over a piece's voxels, c = 2p + 1
MOMENTS_DTYPE = np.dtype([("voxels", "<u8"), ("s1", "<u8", 3), ("s2", "<u8", 6)])
# vrc_affine as a numpy record, for arrays of maps (Affine below is the same 64 bytes as a ctypes structure)
AFFINE_DTYPE = np.dtype([("m", "<i4", 9), ("reserved", "<i4"), ("t", "<i8", 3)])
assert MOMENTS_DTYPE.itemsize == 80 and AFFINE_DTYPE.itemsize == 64
# vrc_piece_contact (include/vrc.h): a posed piece against a world -- its voxel count, and count, sum of c = 2p + 1 and sum of
# normals over the voxels inside the world's solid (overlap) and over those face to face with it (touch)
CONTACT_DTYPE = np.dtype([("posed", "<u8"), ("overlap", "<u8"), ("overlap_s1", "<u8", 3), ("overlap_n", "<i8", 3),
                          ("touch", "<u8"), ("touch_s1", "<u8", 3), ("touch_n", "<i8", 3), ("reserved", "<u8")])
assert CONTACT_DTYPE.itemsize == 128
# vrc_piece_clearance (include/vrc.h): a field read at the voxels of a posed piece -- their count, how many hold
# VRC_DISTANCE_NONE, the sum of the finite values, and the least and greatest one with the voxel that holds it
CLEARANCE_DTYPE = np.dtype([("posed", "<u8"), ("none", "<u8"), ("sum", "<u8"), ("min_value", "<u4"), ("min_at", "<u4", 3),
                            ("max_value", "<u4"), ("max_at", "<u4", 3), ("reserved", "<u8")])
assert CLEARANCE_DTYPE.itemsize == 64
# vrc_sight (include/vrc.h: vrc_sight_segments): a straight walk over a field -- whether it was clear, blocked or had an endpoint
# outside, the first voxel that was not clear (the end of a clear walk) and the voxel visited just before it
SIGHT_DTYPE = np.dtype([("status", "<u4"), ("at", "<u4", 3), ("before", "<u4", 3), ("reserved", "<u4")])
assert SIGHT_DTYPE.itemsize == 32
# a record of a delta (include/vrc.h: vrc_delta_diff): bits = before[word] ^ after[word] != 0, word strictly ascending
DELTA_RECORD_DTYPE = np.dtype([("word", "<u4"), ("bits", "<u4")])
assert DELTA_RECORD_DTYPE.itemsize == 8
# vrc_column (include/vrc.h: vrc_columns_profile): a column met along a direction -- the coordinate of its first and last solid
# voxel (VRC_COLUMN_NONE in an empty one), its solid voxels and its runs of consecutive solid voxels
COLUMN_DTYPE = np.dtype([("first", "<u4"), ("last", "<u4"), ("count", "<u4"), ("runs", "<u4")])
assert COLUMN_DTYPE.itemsize == 16


class VrcError(RuntimeError):
    pass


class Camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("rot", C.c_float * 9),
                ("fov", C.c_float), ("aperture", C.c_float), ("focal_length", C.c_float)]


class FrameParams(C.Structure):
    _fields_ = [("light_position", C.c_float * 3),
                ("use_gi", C.c_uint32), ("use_samples", C.c_uint32),
                ("shadow_samples", C.c_uint32), ("gi_bounces", C.c_uint32),
                ("checker_parity", C.c_int32), ("spp", C.c_uint32),
                ("seed", C.c_uint32), ("frame_index", C.c_uint32),
                ("row_block", C.c_uint32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


class FrameStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("sum_complexity", C.c_uint64),
                ("primary_hits", C.c_uint64), ("pixels", C.c_uint64), ("iterations_not_executed", C.c_uint64)]


class FloodStats(C.Structure):
    _fields_ = [("reached", C.c_uint64), ("sweeps", C.c_uint32), ("converged", C.c_uint32)]


class DistanceStats(C.Structure):
    _fields_ = [("features", C.c_uint64), ("max_d2", C.c_uint32), ("argmax", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class TravelStats(C.Structure):
    """vrc_travel_stats (include/vrc.h): what vrc_travel_field reports"""
    _fields_ = [("seeds", C.c_uint64), ("reached", C.c_uint64), ("max_steps", C.c_uint32), ("argmax", C.c_uint32 * 3),
                ("sweeps", C.c_uint32), ("reserved", C.c_uint32)]


class SightStats(C.Structure):
    """vrc_sight_stats (include/vrc.h): what vrc_sight_field reports"""
    _fields_ = [("visible", C.c_uint64), ("max_d2", C.c_uint32), ("argmax", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class FallStats(C.Structure):
    """vrc_fall_stats (include/vrc.h): what vrc_fall_drops reports"""
    _fields_ = [("moved_voxels", C.c_uint64), ("pieces", C.c_uint32), ("moved_pieces", C.c_uint32), ("max_drop", C.c_uint32),
                ("rounds", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class DeltaStats(C.Structure):
    """vrc_delta_stats (include/vrc.h): the records, the changed voxels and their box (hi exclusive) of a delta"""
    _fields_ = [("words", C.c_uint64), ("voxels", C.c_uint64), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("reserved", C.c_uint32 * 2)]


class PackInfo(C.Structure):
    """vrc_pack_info (include/vrc.h): the header fields of a sparse tile stream -- what vrc_pack_volume wrote or would write"""
    _fields_ = [("depth", C.c_uint32), ("tiles", C.c_uint32), ("mixed_tiles", C.c_uint32), ("full_tiles", C.c_uint32),
                ("partial_bricks", C.c_uint32), ("reserved", C.c_uint32), ("bytes", C.c_uint64), ("solid", C.c_uint64)]


class Affine(C.Structure):
    """vrc_affine (include/vrc.h): the inverse map of vrc_volume_stamp_affine, m row-major with 16 fractional bits"""
    _fields_ = [("m", C.c_int32 * 9), ("reserved", C.c_int32), ("t", C.c_int64 * 3)]


class PieceContact(C.Structure):
    """vrc_piece_contact (include/vrc.h): the same 128 bytes as CONTACT_DTYPE"""
    _fields_ = [("posed", C.c_uint64), ("overlap", C.c_uint64), ("overlap_s1", C.c_uint64 * 3), ("overlap_n", C.c_int64 * 3),
                ("touch", C.c_uint64), ("touch_s1", C.c_uint64 * 3), ("touch_n", C.c_int64 * 3), ("reserved", C.c_uint64)]


# every symbol include/vrc.h declares: (restype, argtypes)
_vp, _u32, _u64, _i32, _f32, _int = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_float, C.c_int
SYMBOLS = {
    "vrc_last_error": (C.c_char_p, []),
    "vrc_device_count": (_int, []),
    "vrc_scene_create": (_int, [_vp, _u64, _u32, _int, C.POINTER(_vp)]),
    "vrc_scene_set_textures": (_int, [_vp, _vp, _vp]),
    "vrc_scene_destroy": (_int, [_vp]),
    "vrc_scene_node_count": (_u64, [_vp]),
    "vrc_scene_depth": (_u32, [_vp]),
    "vrc_build_terrain_lsvo": (_int, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u64)]),
    "vrc_build_volume_lsvo": (_int, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u64)]),
    "vrc_free_host": (None, [_vp]),
    "vrc_scene_build_terrain": (_int, [_vp, _u32, _int, C.POINTER(_vp), C.POINTER(C.c_float)]),
    "vrc_scene_build_volume": (_int, [_vp, _u32, _int, C.POINTER(_vp), C.POINTER(C.c_float)]),
    "vrc_scene_download_nodes": (_int, [_vp, _vp]),
    "vrc_terrain_heights": (_int, [_i32, _u32, _int, _vp]),
    "vrc_scene_build_fastnoise_terrain": (_int, [_i32, _u32, _int, C.POINTER(_vp), C.POINTER(C.c_float)]),
    "vrc_cast_rays": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "vrc_cast_ray_chains": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp]),
    "vrc_cast_ray": (_int, [_vp, _vp, _vp, _f32, _f32, _vp]),
    "vrc_grid_create": (_int, [_vp, _i32, _i32, _i32, _int, C.POINTER(_vp)]),
    "vrc_grid_destroy": (_int, [_vp]),
    "vrc_grid_cast_rays": (_int, [_vp, _u64, _vp, _vp, _vp, _int, _vp]),
    "vrc_renderer_create": (_int, [_vp, _u32, _u32, C.POINTER(_vp)]),
    "vrc_renderer_destroy": (_int, [_vp]),
    "vrc_render_frame": (_int, [_vp, C.POINTER(Camera), C.POINTER(FrameParams), _vp]),
    "vrc_render_frame_resolved": (_int, [_vp, C.POINTER(Camera), C.POINTER(FrameParams), _vp, _vp]),
    "vrc_renderer_set_primary_capture": (_int, [_vp, _vp]),
    "vrc_samples_to_image": (_int, [_vp, _vp]),
    "vrc_reset_samples": (_int, [_vp, _vp]),
    "vrc_clear_image": (_int, [_vp, _vp]),
    "vrc_image_device_ptr": (_vp, [_vp]),
    "vrc_accum_device_ptr": (_vp, [_vp]),
    "vrc_read_image": (_int, [_vp, _vp, _vp]),
    "vrc_write_image": (_int, [_vp, _vp, _vp]),
    "vrc_read_accum": (_int, [_vp, _vp, _vp]),
    "vrc_get_stats": (_int, [_vp, C.POINTER(FrameStats), _int, _vp]),
    "vrc_shard_bytes": (_u64, [_u32, _u32, _u32, _u32]),
    "vrc_pack_shard": (_int, [_vp, _u32, _u32, _u32, _vp, _vp]),
    "vrc_resolve_shard": (_int, [_vp, _u32, _u32, _u32, _vp, _int, _vp]),
    "vrc_unpack_shards": (_int, [_vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "vrc_make_rotation": (None, [_f32, _f32, _vp]),
    "vrc_set_tuning": (_int, [_u32]),
    "vrc_presenter_create": (_int, [_int, _u32, _u32, _u32, _u32, C.POINTER(_vp)]),
    "vrc_presenter_destroy": (_int, [_vp]),
    "vrc_present": (_int, [_vp, _vp, _f32, _u32, _vp]),
    "vrc_present_image": (_int, [_vp, _vp, _f32, _u32, _vp]),
    "vrc_presenter_clear": (_int, [_vp, _vp]),
    "vrc_presenter_window_ptr": (_vp, [_vp]),
    "vrc_presenter_denoised_ptr": (_vp, [_vp]),
    "vrc_presenter_read": (_int, [_vp, _vp, _vp, _vp]),
    "vrc_selftest_exact_arith": (_int, [_int, _vp]),
    "vrc_set_sample_chunk": (_int, [_u32]),
    "vrc_renderer_set_tuning": (_int, [_vp, _u32]),
    "vrc_renderer_set_sample_chunk": (_int, [_vp, _u32]),
    "vrc_renderer_set_invariant_ray_reuse": (_int, [_vp, _u32]),
    "vrc_renderer_set_walk_from_root": (_int, [_vp, _u32]),
    "vrc_renderer_set_lane_samples": (_int, [_vp, _u32]),
    "vrc_set_lane_samples": (_int, [_u32]),
    "vrc_renderer_set_quad_walks": (_int, [_vp, _u32]),
    "vrc_renderer_last_kernel": (C.c_char_p, [_vp]),
    "vrc_ipc_export_image": (_int, [_vp, _vp]),
    "vrc_ipc_open_image": (_int, [_int, _vp, C.POINTER(_vp)]),
    "vrc_ipc_close_image": (_int, [_int, _vp]),
    "vrc_renderer_set_image_target": (_int, [_vp, _vp]),
    "vrc_ipc_flags_open": (_int, [C.c_char_p, _u32, _int, _int, C.POINTER(_vp)]),
    "vrc_ipc_flags_close": (_int, [_vp]),
    "vrc_ipc_flags_unlink": (_int, [_vp]),
    "vrc_ipc_stream_wait": (_int, [_vp, _vp, _vp, _u32, _u32]),
    "vrc_ipc_flag_set": (_int, [_vp, _u32, _u32]),
    "vrc_stream_write_flag": (_int, [_vp, _u32, _u32, _vp]),
    "vrc_stream_wait_flag": (_int, [_vp, _u32, _u32, _vp]),
    "vrc_ipc_flag_value": (_u32, [_vp, _u32]),
    "vrc_stream_create": (_int, [_int, C.POINTER(_vp)]),
    "vrc_stream_destroy": (_int, [_int, _vp]),
    "vrc_stream_synchronize": (_int, [_int, _vp]),
    "vrc_volume_create": (_int, [_u32, _int, C.POINTER(_vp)]),
    "vrc_volume_from_scene": (_int, [_vp, C.POINTER(_vp)]),
    "vrc_volume_destroy": (_int, [_vp]),
    "vrc_volume_depth": (_u32, [_vp]),
    "vrc_volume_set_voxels": (_int, [_vp, _u64, _vp, _int, _int, _vp]),
    "vrc_volume_fill_boxes": (_int, [_vp, _u64, _vp, _int, _int, _vp]),
    "vrc_volume_commit": (_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_float)]),
    "vrc_volume_download": (_int, [_vp, _vp]),
    "vrc_volume_solid_count": (_int, [_vp, C.POINTER(_u64)]),
    "vrc_volume_fill_spheres": (_int, [_vp, _u64, _vp, _int, _int, _vp]),
    "vrc_volume_fill_spheres_at_hits": (_int, [_vp, _u64, _vp, _i32, _int, _int, _vp]),
    "vrc_stroke_fill_capsules": (_int, [_vp, _u64, _vp, _int, _int, _vp]),
    "vrc_stroke_fill_at_hits": (_int, [_vp, _u64, _vp, _i32, _u32, _int, _int, _vp]),
    "vrc_volume_copy_region": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "vrc_volume_stamp_affine": (_int, [_vp, _vp, C.POINTER(Affine), _vp, _vp, _int, _vp]),
    "vrc_affine_place": (_int, [_vp, _f32, _vp, _vp, _u32, _u32, C.POINTER(Affine), _vp, _vp]),
    "vrc_affine_place_box": (_int, [_vp, _f32, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "vrc_volume_clone": (_int, [_vp, C.POINTER(_vp)]),
    "vrc_volume_get_voxels": (_int, [_vp, _u64, _vp, _vp, _int, _vp]),
    "vrc_volume_count_boxes": (_int, [_vp, _u64, _vp, _vp, _int, _vp]),
    "vrc_volume_flood": (_int, [_vp, _vp, _int, _int, _u32, C.POINTER(FloodStats)]),
    "vrc_volume_label_components": (_int, [_vp, _int, _int, C.POINTER(_vp), C.POINTER(_u64)]),
    "vrc_labels_destroy": (_int, [_vp]),
    "vrc_labels_count": (_u64, [_vp]),
    "vrc_labels_depth": (_u32, [_vp]),
    "vrc_labels_bytes": (_u64, [_vp]),
    "vrc_labels_components": (_int, [_vp, _u64, _u64, _vp, _int, _vp]),
    "vrc_labels_at": (_int, [_vp, _u64, _vp, _vp, _int, _vp]),
    "vrc_labels_select": (_int, [_vp, _vp, _vp, _int, _int, _vp]),
    "vrc_fall_drops": (_int, [_vp, _vp, _int, _u32, _vp, _int, C.POINTER(FallStats)]),
    "vrc_fall_place": (_int, [_vp, _vp, _vp, _vp, _int, _int, _vp]),
    "vrc_fracture_label": (_int, [_vp, _int, _int, _u64, _vp, _u32, _int, C.POINTER(_vp), C.POINTER(_u64)]),
    "vrc_fracture_piece_sites": (_int, [_vp, _u64, _u64, _vp, _int, _vp]),
    "vrc_rigid_moments": (_int, [_vp, _u64, _u64, _vp, _int, _vp]),
    "vrc_rigid_place_affine": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    "vrc_rigid_contacts": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "vrc_rigid_pair_contacts": (_int, [_vp, _vp, _vp, _vp, _u32, _u64, _vp, _vp, _int, _vp]),
    "vrc_rigid_clearance": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "vrc_rigid_box_pair_count": (_int, [_vp, _vp, _vp, _u32, C.POINTER(_u64), _int, _vp]),
    "vrc_rigid_box_pairs": (_int, [_vp, _vp, _vp, _u32, _u64, _u64, _vp, _int, _vp]),
    "vrc_volume_distance_field": (_int, [_vp, _int, _int, C.POINTER(_vp), C.POINTER(DistanceStats)]),
    "vrc_distance_destroy": (_int, [_vp]),
    "vrc_distance_depth": (_u32, [_vp]),
    "vrc_distance_bytes": (_u64, [_vp]),
    "vrc_distance_data": (_vp, [_vp]),
    "vrc_distance_at": (_int, [_vp, _u64, _vp, _vp, _int, _vp]),
    "vrc_distance_download": (_int, [_vp, _vp]),
    "vrc_distance_select": (_int, [_vp, _u32, _u32, _vp, _int, _vp]),
    "vrc_travel_field": (_int, [_vp, _vp, _int, _int, _u32, C.POINTER(_vp), C.POINTER(TravelStats)]),
    "vrc_travel_connectivity": (_int, [_vp]),
    "vrc_travel_trace_paths": (_int, [_vp, _u64, _vp, _u32, _vp, _vp, _int, _vp]),
    "vrc_sight_segments": (_int, [_vp, _u64, _vp, _u32, _u32, _int, _vp, _int, _vp]),
    "vrc_sight_field": (_int, [_vp, _vp, _u32, _u32, _u32, _int, C.POINTER(_vp), C.POINTER(SightStats)]),
    "vrc_delta_diff": (_int, [_vp, _vp, C.POINTER(_vp), C.POINTER(DeltaStats)]),
    "vrc_delta_create": (_int, [_u32, _int, _u64, _vp, _int, C.POINTER(_vp), C.POINTER(DeltaStats)]),
    "vrc_delta_destroy": (_int, [_vp]),
    "vrc_delta_count": (_u64, [_vp]),
    "vrc_delta_depth": (_u32, [_vp]),
    "vrc_delta_bytes": (_u64, [_vp]),
    "vrc_delta_get_stats": (_int, [_vp, C.POINTER(DeltaStats)]),
    "vrc_delta_records": (_int, [_vp, _u64, _u64, _vp, _int, _vp]),
    "vrc_delta_apply": (_int, [_vp, _vp, _vp]),
    "vrc_pack_bound": (_u64, [_u32]),
    "vrc_pack_header": (_int, [_vp, _u64, C.POINTER(PackInfo)]),
    "vrc_pack_volume": (_int, [_vp, _vp, _u64, C.POINTER(PackInfo), _int]),
    "vrc_unpack_volume": (_int, [_vp, _vp, _u64, _int]),
    "vrc_cells_step": (_int, [_vp, _vp, _int, _u32, _u32, _int, _vp, _int, _vp]),
    "vrc_cells_fill_random": (_int, [_vp, _u32, _u64, _vp, _int, _vp]),
    "vrc_columns_profile": (_int, [_vp, _int, _vp, _vp, _int, _vp]),
    "vrc_columns_fill": (_int, [_vp, _int, _vp, _vp, _i32, _vp, _i32, _int, _int, _vp]),
    "vrc_columns_select": (_int, [_vp, _vp, _int, _u32, _u32, _int, _int, _vp]),
    "vrc_levels_counts": (_int, [_vp, _u32, _vp, _int, _vp]),
    "vrc_levels_reduce": (_int, [_vp, _vp, _u32, _u32, _int, _vp]),
    "vrc_levels_expand": (_int, [_vp, _vp, _int, _vp]),
    "vrc_morph_apply": (_int, [_vp, _vp, _int, _int, _u64, _vp, _vp, _int, _int, _int, _vp]),
    "vrc_volume_xor_mesh": (_int, [_vp, _u64, _vp, _int, _vp]),
    "vrc_raster_mesh": (_int, [_vp, _u64, _vp, _int, _int, _int, _vp]),
    "vrc_volume_surface_count": (_int, [_vp, _int, _vp]),
    "vrc_volume_extract_surface": (_int, [_vp, _int, _int, _u64, _u64, _vp, _vp, _int, _vp]),
    "vrc_rect_count": (_int, [_vp, _int, _vp]),
    "vrc_extract_rects": (_int, [_vp, _int, _int, _u64, _u64, _vp, _vp, _int, _vp]),
    "vrc_voxels_count": (_int, [_vp, _int, _int, _vp, C.POINTER(_u64)]),
    "vrc_voxels_extract": (_int, [_vp, _int, _int, _vp, _int, _u64, _u64, _vp, _vp, _int, _vp]),
    "vrc_volume_edit_scratch_bytes": (_int, [_vp, C.POINTER(_u64)]),
    "vrc_renderer_set_scene": (_int, [_vp, _vp]),
    "vrc_hit_to_voxel": (_int, [_u32, _vp, _vp, _vp, C.POINTER(_int)]),
}

_lib = None


def load():
    """Load libvrc_hip.so; raises VrcError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # PyTorch bundles its own libamdhip64; it must be the HIP runtime of the
        # process (loading /opt/rocm's first makes torch see "No HIP GPUs").
        import torch  # noqa: F401
    except ImportError:
        pass
    path = LIB_PATH
    variant = os.environ.get("VRC_LIB", "").strip()
    if variant:
        # an EXPERIMENT build of the same sources (tools/build_variant.py -> gpurun_variants/var_<name>.so) loaded in the
        # product's place for an A/B -- never by overwriting the product library; said out loud, and bench.py records it
        if not os.path.exists(variant):
            raise VrcError(f"VRC_LIB={variant} does not exist")
        import sys
        print(f"cpuvoxelraycaster_amd: VRC_LIB set -- loading the experiment library {variant}, not the product {LIB_PATH}", file=sys.stderr)
        path = variant
    if not os.path.exists(path):
        raise VrcError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(the HIP library is the product; there is no fallback)")
    L = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise VrcError(f"vrc error {rc}: {load().vrc_last_error().decode()}")


def ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, C.c_void_p):
        return a
    return C.c_void_p(int(a))  # raw device pointer (e.g. torch tensor .data_ptr())


def make_rotation(angle_x, angle_y):
    rot = np.zeros(9, np.float32)
    load().vrc_make_rotation(angle_x, angle_y, ptr(rot))
    return rot


def _take_host_nodes(out, n):
    arr = np.frombuffer((C.c_uint8 * (n.value * 8)).from_address(out.value), dtype=LNODE_DTYPE).copy()
    load().vrc_free_host(out)
    return arr


def build_terrain_lsvo(height_i32, depth):
    size = 1 << depth
    h = np.ascontiguousarray(np.asarray(height_i32)[:size, :size], dtype=np.int32)
    out, n = C.c_void_p(), C.c_uint64()
    check(load().vrc_build_terrain_lsvo(ptr(h), depth, C.byref(out), C.byref(n)))
    return _take_host_nodes(out, n)


def build_volume_lsvo(solid_u8, depth):
    size = 1 << depth
    s = np.ascontiguousarray(solid_u8, dtype=np.uint8)
    assert s.shape == (size, size, size)
    out, n = C.c_void_p(), C.c_uint64()
    check(load().vrc_build_volume_lsvo(ptr(s), depth, C.byref(out), C.byref(n)))
    return _take_host_nodes(out, n)
