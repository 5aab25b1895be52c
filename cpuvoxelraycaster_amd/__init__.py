"""MI355X-native voxel ray traversal: the LSVO::castRay / RayCaster hot path of
johnBuffer/CpuVoxelRaycaster as hand-written HIP kernels behind a C ABI
(include/vrc.h).  See DESIGN.md."""
from . import capi
from .capi import VrcError, HIT_DTYPE, LNODE_DTYPE, COMPONENT_DTYPE, SIGHT_DTYPE, DELTA_RECORD_DTYPE, build_terrain_lsvo, build_volume_lsvo, make_rotation
from .raycaster import LSVO, Grid3D, RayCaster, Presenter, VoxelVolume, VoxelLabels, VoxelDistance, VoxelDelta, VoxelHistory, smoothPath, packed_info, hit_to_voxel, make_camera, make_affine, affine_place, affine_place_box, affine_signed_permutation, mass_properties, contact_properties, free_radius, count_mask, count_range, neighbour_bit, face_exposure, corner_occlusion, element_ball, element_box, element_cross, element_line, element_of, reflect
from .scenes import terrain_heights, load_textures, load_bmp, load_textures_bmp, reference_camera, reference_camera_position, reference_light, icosphere, box_mesh, write_obj, scatter_sites

__all__ = ["capi", "VrcError", "HIT_DTYPE", "LNODE_DTYPE", "build_terrain_lsvo", "build_volume_lsvo",
           "make_rotation", "LSVO", "Grid3D", "RayCaster", "Presenter", "VoxelVolume", "VoxelLabels", "VoxelDistance", "VoxelDelta", "VoxelHistory", "smoothPath", "packed_info", "COMPONENT_DTYPE", "SIGHT_DTYPE", "DELTA_RECORD_DTYPE", "hit_to_voxel", "make_camera", "make_affine", "affine_place", "affine_place_box", "affine_signed_permutation", "mass_properties", "contact_properties", "free_radius", "count_mask", "count_range", "neighbour_bit", "face_exposure", "corner_occlusion", "element_ball", "element_box", "element_cross", "element_line", "element_of", "reflect", "terrain_heights", "load_bmp", "load_textures_bmp",
           "load_textures", "reference_camera", "reference_camera_position", "reference_light", "scatter_sites"]
