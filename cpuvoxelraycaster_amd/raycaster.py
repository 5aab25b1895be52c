"""Thin Python mirror of the reference's operator interface for the hot path,
over the C ABI (include/vrc.h).  Names follow the reference:

  LSVO.castRay                 <- LSVO<N>::castRay          (include/lsvo.hpp:33)
  RayCaster.setLightPosition   <- RayCaster::setLightPosition (include/raycaster.hpp:62)
  RayCaster.renderFrame        <- the swarm lambda: getRay + renderRay per pixel (src/main.cpp:139-152)
  RayCaster.samples_to_image   <- raycaster.hpp:94
  RayCaster.resetSamples       <- raycaster.hpp:105
  VoxelVolume.setVoxels        <- Volumetric::setCell       (include/volumetric.hpp:59), batched; commit() -> a new LSVO
  Presenter.present            <- the SFML blend / upscale chain after the frame (src/main.cpp:160-182)

All compute runs in the HIP kernels of libvrc_hip.so; numpy / torch are only
used to hold buffers."""
import ctypes as C

import numpy as np

from . import capi
from .capi import Camera, FrameParams, FrameStats, HIT_DTYPE, VrcError, check, ptr


class LSVO:
    """Device-resident linear sparse voxel octree (Volumetric implementation)."""

    def __init__(self, lnodes, depth, device=0, textures=None):
        L = capi.load()
        lnodes = np.ascontiguousarray(lnodes)
        if lnodes.dtype.itemsize != 8:
            raise VrcError("lnodes must be an array of 8-byte LNode records")
        self._h = C.c_void_p()
        check(L.vrc_scene_create(ptr(lnodes), lnodes.shape[0], depth, device, C.byref(self._h)))
        self.depth = depth
        self.device = device
        self.n_nodes = int(lnodes.shape[0])
        if textures is not None:
            self.setTextures(*textures)

    @classmethod
    def _from_handle(cls, handle, depth, device, textures):
        self = cls.__new__(cls)
        self._h = handle
        self.depth, self.device = depth, device
        self.n_nodes = int(capi.load().vrc_scene_node_count(handle))
        self.build_ms = None
        if textures is not None:
            self.setTextures(*textures)
        return self

    @classmethod
    def fromTerrain(cls, height_i32, depth, device=0, textures=None):
        """Build the LSVO of the reference's terrain generator on the GPU (main.cpp:59-88)."""
        size = 1 << depth
        h = np.ascontiguousarray(np.asarray(height_i32)[:size, :size], dtype=np.int32)
        handle, ms = C.c_void_p(), C.c_float()
        check(capi.load().vrc_scene_build_terrain(ptr(h), depth, device, C.byref(handle), C.byref(ms)))
        self = cls._from_handle(handle, depth, device, textures)
        self.build_ms = ms.value
        return self

    @classmethod
    def fromFastNoiseTerrain(cls, depth, seed=1337, device=0, textures=None):
        """main.cpp:59-88 end to end on the GPU: FastNoise heights -> LSVO."""
        handle, ms = C.c_void_p(), C.c_float()
        check(capi.load().vrc_scene_build_fastnoise_terrain(seed, depth, device, C.byref(handle), C.byref(ms)))
        self = cls._from_handle(handle, depth, device, textures)
        self.build_ms = ms.value
        return self

    @classmethod
    def fromVolume(cls, solid_u8, depth, device=0, textures=None):
        """Build the LSVO of an arbitrary occupancy volume solid[x, y, z] on the GPU."""
        size = 1 << depth
        s = np.ascontiguousarray(solid_u8, dtype=np.uint8)
        assert s.shape == (size, size, size)
        handle, ms = C.c_void_p(), C.c_float()
        check(capi.load().vrc_scene_build_volume(ptr(s), depth, device, C.byref(handle), C.byref(ms)))
        self = cls._from_handle(handle, depth, device, textures)
        self.build_ms = ms.value
        return self

    def downloadNodes(self):
        out = np.zeros(self.n_nodes, capi.LNODE_DTYPE)
        check(capi.load().vrc_scene_download_nodes(self._h, ptr(out)))
        return out

    def setTextures(self, top_rgb, side_rgb):
        top = np.ascontiguousarray(top_rgb, dtype=np.uint8).reshape(-1)
        side = np.ascontiguousarray(side_rgb, dtype=np.uint8).reshape(-1)
        assert top.size == 768 and side.size == 768
        check(capi.load().vrc_scene_set_textures(self._h, ptr(top), ptr(side)))

    def castRay(self, position, direction, ray_size_coef=0.0, ray_size_bias=0.0):
        """Single ray (Camera::getClosestPoint path); returns a HIT_DTYPE record."""
        out = np.zeros(1, HIT_DTYPE)
        o = np.ascontiguousarray(position, np.float32)
        d = np.ascontiguousarray(direction, np.float32)
        check(capi.load().vrc_cast_ray(self._h, ptr(o), ptr(d), ray_size_coef, ray_size_bias, ptr(out)))
        return out[0]

    def castRays(self, org, dir_, coef=None, bias=None):
        """Batch form over host arrays."""
        org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
        dir_ = np.ascontiguousarray(dir_, np.float32).reshape(-1, 3)
        n = org.shape[0]
        if coef is not None:
            coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, np.float32), (n,)))
        if bias is not None:
            bias = np.ascontiguousarray(np.broadcast_to(np.asarray(bias, np.float32), (n,)))
        out = np.zeros(n, HIT_DTYPE)
        check(capi.load().vrc_cast_rays(self._h, n, ptr(org), ptr(dir_), ptr(coef), ptr(bias), ptr(out),
                                        capi.VRC_MEM_HOST, None))
        return out

    def castRaysDevice(self, n, org_ptr, dir_ptr, out_ptr, coef_ptr=None, bias_ptr=None, stream=None):
        """Batch form over device pointers (asynchronous on `stream`)."""
        check(capi.load().vrc_cast_rays(self._h, n, ptr(org_ptr), ptr(dir_ptr), ptr(coef_ptr), ptr(bias_ptr),
                                        ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def castRayChainsDevice(self, n, org_a_ptr, dir_a_ptr, org_b_ptr, dir_b_ptr, coef_b, out_a_ptr, out_b_ptr, not_executed_ptr=None, stream=None):
        """ray A from the root, then ray B started below the root next to A's hit (include/vrc.h: vrc_cast_ray_chains)"""
        check(capi.load().vrc_cast_ray_chains(self._h, n, ptr(org_a_ptr), ptr(dir_a_ptr), ptr(org_b_ptr), ptr(dir_b_ptr), float(coef_b),
                                              ptr(out_a_ptr), ptr(out_b_ptr), ptr(not_executed_ptr), ptr(stream)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hit_to_voxel(depth, hit):
    """The voxel a castRay record hit, in setCell coordinates, and the empty cell the ray came through (None when there is
    none): ((x, y, z), (x, y, z) | None).  Host arithmetic (include/vrc.h: vrc_hit_to_voxel); raises for a miss / LOD cut-off."""
    rec = np.zeros(1, HIT_DTYPE)
    rec[0] = hit
    voxel, neighbour, has = np.zeros(3, np.uint32), np.zeros(3, np.uint32), C.c_int()
    check(capi.load().vrc_hit_to_voxel(depth, ptr(rec), ptr(voxel), ptr(neighbour), C.byref(has)))
    return tuple(int(v) for v in voxel), (tuple(int(v) for v in neighbour) if has.value else None)


def make_affine(m, t):
    """capi.Affine from 9 row-major int32 (16 fractional bits) and 3 int64 (units of 2^-17 voxel)"""
    a = capi.Affine()
    m, t = [int(v) for v in np.asarray(m, object).reshape(9)], [int(v) for v in np.asarray(t, object).reshape(3)]
    for i in range(9):
        a.m[i] = m[i]
    for i in range(3):
        a.t[i] = t[i]
    return a


def affine_signed_permutation(perm, flip, size):
    """The exact integer map of VoxelVolume.stampAffine for q_a = p[perm[a]], or size-1 - p[perm[a]] where flip[a] is set: one
    of the 48 turns and mirrorings of a cube of `size` voxels.  It maps voxel centres to voxel centres."""
    m, t = [0] * 9, [0] * 3
    for a in range(3):
        m[3 * a + int(perm[a])] = -65536 if flip[a] else 65536
        t[a] = (int(size) << 17) if flip[a] else 0
    return make_affine(m, t)


def affine_place(rot, scale, src_pivot, dst_pivot, src_depth, dst_depth):
    """(capi.Affine, lo, hi): the inverse map and the destination box of the placement
    x_dst = dst_pivot + scale * R * (x_src - src_pivot), rot in make_rotation's layout.  Host arithmetic (include/vrc.h:
    vrc_affine_place); raises for a scale below 1/16 or non-finite input."""
    rot = np.ascontiguousarray(rot, np.float32).reshape(9)
    sp, dp = np.ascontiguousarray(src_pivot, np.float32).reshape(3), np.ascontiguousarray(dst_pivot, np.float32).reshape(3)
    a, lo, hi = capi.Affine(), np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    check(capi.load().vrc_affine_place(ptr(rot), float(scale), ptr(sp), ptr(dp), int(src_depth), int(dst_depth), C.byref(a), ptr(lo), ptr(hi)))
    return a, tuple(int(v) for v in lo), tuple(int(v) for v in hi)


def affine_place_box(rot, scale, src_pivot, dst_pivot, src_lo, src_hi, dst_depth):
    """affine_place for a part of the source, the voxel box [src_lo, src_hi) -- a piece by its record box -- in place of the
    whole cube (include/vrc.h: vrc_affine_place_box).  Returns (capi.Affine, lo, hi)."""
    rot = np.ascontiguousarray(rot, np.float32).reshape(9)
    sp, dp = np.ascontiguousarray(src_pivot, np.float32).reshape(3), np.ascontiguousarray(dst_pivot, np.float32).reshape(3)
    slo, shi = np.ascontiguousarray(src_lo, np.uint32).reshape(3), np.ascontiguousarray(src_hi, np.uint32).reshape(3)
    a, lo, hi = capi.Affine(), np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    check(capi.load().vrc_affine_place_box(ptr(rot), float(scale), ptr(sp), ptr(dp), ptr(slo), ptr(shi), int(dst_depth), C.byref(a), ptr(lo), ptr(hi)))
    return a, tuple(int(v) for v in lo), tuple(int(v) for v in hi)


def affine_array(maps):
    """a sequence of capi.Affine (or an array of capi.AFFINE_DTYPE) as one contiguous capi.AFFINE_DTYPE array"""
    if isinstance(maps, np.ndarray) and maps.dtype == capi.AFFINE_DTYPE:
        return np.ascontiguousarray(maps).reshape(-1)
    out = np.zeros(len(maps), capi.AFFINE_DTYPE)
    for i, a in enumerate(maps):
        out[i] = (list(a.m), a.reserved, list(a.t))
    return out


def mass_properties(moments):
    """(mass, centre, inertia) as float64 arrays of shapes (k,), (k, 3), (k, 3, 3) from k capi.MOMENTS_DTYPE records
    (include/vrc.h: vrc_rigid_moments).  A voxel is a unit cube of unit mass: mass n, centre of mass s1 / (2n) in continuous
    voxel coordinates, and about it I_aa = sum(r_b^2 + r_c^2) + n/6, I_ab = -sum(r_a r_b).  Every entry is the exact rational
    value of the integer sums, rounded once to float64."""
    from fractions import Fraction
    moments = np.asarray(moments, capi.MOMENTS_DTYPE).reshape(-1)
    k = len(moments)
    mass, centre, inertia = np.zeros(k), np.zeros((k, 3)), np.zeros((k, 3, 3))
    pair = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}
    for i, rec in enumerate(moments):
        n = int(rec["voxels"])
        if n == 0:
            continue
        s1 = [int(v) for v in rec["s1"]]
        s2 = [int(v) for v in rec["s2"]]
        # sum of r_a r_b about the centre of mass, r = c / 2 - s1 / (2n): (n s2_ab - s1_a s1_b) / (4n)
        central = {ab: Fraction(n * s2[j] - s1[ab[0]] * s1[ab[1]], 4 * n) for ab, j in pair.items()}
        mass[i] = float(n)
        for a in range(3):
            centre[i, a] = float(Fraction(s1[a], 2 * n))
            b, c = (a + 1) % 3, (a + 2) % 3
            inertia[i, a, a] = float(central[(b, b)] + central[(c, c)] + Fraction(n, 6))
        for (a, b) in ((0, 1), (0, 2), (1, 2)):
            inertia[i, a, b] = inertia[i, b, a] = float(-central[(a, b)])
    return mass, centre, inertia


def contact_properties(records):
    """(overlap_centre, overlap_normal, touch_centre, touch_normal) as float64 arrays of shape (k, 3) from k
    capi.CONTACT_DTYPE records (include/vrc.h: vrc_rigid_contacts).  A centre is the centroid s1 / (2 count) of the set in
    continuous voxel coordinates, the exact rational value rounded once; a normal is the unit vector n / |n| of the summed
    voxel normals, pointing from the solid into the open.  Zeros where the count or the vector is zero."""
    from fractions import Fraction
    from math import isqrt
    records = np.asarray(records, capi.CONTACT_DTYPE).reshape(-1)
    k = len(records)
    out = [np.zeros((k, 3)) for _ in range(4)]
    for i, rec in enumerate(records):
        for j, name in enumerate(("overlap", "touch")):
            count = int(rec[name])
            if count:
                out[2 * j][i] = [float(Fraction(int(v), 2 * count)) for v in rec[name + "_s1"]]
            n = [int(v) for v in rec[name + "_n"]]
            nn = sum(v * v for v in n)
            if nn:
                # |n| from the integer root of nn scaled to 54 bits or more (nn itself may exceed 2^53), rounded once; with the
                # division the result is within one unit in the last place of n / |n|
                shift = max(0, 54 - nn.bit_length() // 2)
                root = isqrt(nn << (2 * shift))
                length = float(Fraction(root, 1 << shift))
                out[2 * j + 1][i] = [v / length for v in n]
    return tuple(out)


def free_radius(min_value, S):
    """VoxelLabels.freeRadius' rule on an array of vrc_piece_clearance min_value over a squared-distance field of S^3: int64
    isqrt(min_value - 1), the largest r with r^2 < min_value; -1 where min_value is 0; S where it is capi.VRC_DISTANCE_NONE"""
    from math import isqrt
    values = np.asarray(min_value, np.uint32).reshape(-1)
    return np.array([int(S) if v == capi.VRC_DISTANCE_NONE else isqrt(int(v) - 1) if v else -1 for v in values.tolist()], np.int64)


def count_mask(counts):
    """the bit mask of a cell rule (VoxelVolume.cellStep): an int as it is, an iterable of neighbour counts as the OR of
    1 << count"""
    if isinstance(counts, (int, np.integer)):
        return int(counts)
    mask = 0
    for c in counts:
        mask |= 1 << int(c)
    return mask


def count_range(rule, k):
    """the band (lo, hi) of cell counts of level k that a reduction rule keeps (VoxelVolume.reduceInto): "any" is at least one
    of the cell's 8^k voxels, "all" every one, "majority" at least half, "empty" none; a pair (lo, hi) as it is"""
    full = 8 ** int(k)
    if isinstance(rule, str):
        named = {"any": (1, full + 1), "all": (full, full + 1), "majority": (full // 2, full + 1), "empty": (0, 1)}
        if rule not in named:
            raise ValueError(f"count_range: rule {rule!r} is none of {sorted(named)}")
        return named[rule]
    lo, hi = rule
    return int(lo), int(hi)


def _element(offsets):
    return np.ascontiguousarray(offsets, np.int32).reshape(-1, 3)


def element_ball(r):
    """(n, 3) int32: the offsets with d^2 <= r^2, the structuring element of VoxelVolume.dilate(r); r <= 16"""
    r = int(r)
    if r < 0:
        raise ValueError(f"element_ball: negative radius {r}")
    g = np.indices((2 * r + 1,) * 3).reshape(3, -1).T - r
    return _element(g[(g.astype(np.int64) ** 2).sum(axis=1) <= r * r])


def element_box(a, b, c, anchor=None):
    """(a b c, 3) int32: the a x b x c box whose voxel `anchor` is the pivot (a // 2, b // 2, c // 2 by default)"""
    at = (int(a) // 2, int(b) // 2, int(c) // 2) if anchor is None else tuple(int(v) for v in anchor)
    return _element(np.indices((int(a), int(b), int(c))).reshape(3, -1).T - np.array(at))


def element_cross():
    """(7, 3) int32: the pivot and its six face neighbours"""
    return _element([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)])


def element_line(axis, lo, hi):
    """(hi - lo + 1, 3) int32: the offsets lo .. hi (both included) along `axis`; element_line(0, 0, 6) smears 6 voxels along +x"""
    e = np.zeros((max(int(hi) - int(lo) + 1, 0), 3), np.int32)
    e[:, int(axis)] = np.arange(int(lo), int(hi) + 1)
    return e


def element_of(shape, pivot=(0, 0, 0)):
    """(n, 3) int32: the solid voxels of a dense [x, y, z] array or of a VoxelVolume, relative to `pivot`"""
    voxels = shape.voxels() if isinstance(shape, VoxelVolume) else np.argwhere(np.asarray(shape))
    return _element(voxels.astype(np.int64) - np.asarray(pivot, np.int64).reshape(1, 3))


def reflect(element):
    """-E: the element of the dual operation (include/vrc.h: vrc_morph_apply)"""
    return _element(-_element(element))


def packed_info(data):
    """The header of a sparse tile stream (bytes, a uint8 numpy array or a uint8 torch tensor) as a capi.PackInfo, held to
    the header rules of include/vrc.h (vrc_pack_header): pure host, only the first 64 bytes are read."""
    if hasattr(data, "data_ptr"):
        total, head = int(data.numel()), data.reshape(-1)[:64].cpu().numpy()
    elif isinstance(data, (bytes, bytearray, memoryview)):
        total, head = len(data), np.frombuffer(data, np.uint8, min(64, len(data)))
    else:
        flat = np.asarray(data, np.uint8).reshape(-1)
        total, head = flat.size, flat[:64]
    head = np.concatenate([np.ascontiguousarray(head, np.uint8), np.zeros(64 - len(head), np.uint8)])    # a short stream is refused by its length
    info = capi.PackInfo()
    check(capi.load().vrc_pack_header(ptr(head), total, C.byref(info)))
    return info


def neighbour_bit(dx, dy, dz):
    """the bit of a neighbourhood mask (include/vrc.h: VRC_VOXELS_NEIGHBOURS) that holds voxel c + (dx, dy, dz)"""
    if not all(q in (-1, 0, 1) for q in (dx, dy, dz)):
        raise ValueError("dx, dy, dz are -1, 0 or 1")
    return 9 * (dx + 1) + 3 * (dy + 1) + (dz + 1)


def _offset_bit(axis_offsets):
    """neighbour_bit of the offset given as {axis: step}"""
    o = [0, 0, 0]
    for a, q in axis_offsets.items():
        o[a] = q
    return neighbour_bit(*o)


def face_exposure(m):
    """uint8 per neighbourhood mask: bit d is set iff face d = 2 * axis + side (capi.VRC_FACE_*) of the voxel is exposed,
    that is iff the face neighbour on that side is empty.  Host arithmetic."""
    m = np.asarray(m, np.uint32)
    out = np.zeros(m.shape, np.uint8)
    for d in range(6):
        k = _offset_bit({d >> 1: 1 if d & 1 else -1})
        out |= ((((m >> np.uint32(k)) & np.uint32(1)) ^ np.uint32(1)) << np.uint32(d)).astype(np.uint8)
    return out


def corner_occlusion(m, d):
    """(..., 4) uint8: the ambient-occlusion level 0 (darkest) .. 3 (open) at the corners q0 .. q3 of face d of every
    neighbourhood mask, in vrc_volume_extract_surface's corner order.  With side1, side2 and corner the three voxels that
    touch the corner in the layer in front of the face, the level is 0 if side1 and side2 else 3 - (side1 + side2 +
    corner): what a caller of VoxelVolume.meshFromFaces shades its vertices with.  Host arithmetic."""
    if d not in range(6):
        raise ValueError(f"face {d} is not a code 0..5")
    m = np.asarray(m, np.uint32)
    a, front = d >> 1, (1 if d & 1 else -1)
    u, v = (a + 1) % 3, (a + 2) % 3
    out = np.zeros(m.shape + (4,), np.uint8)
    for k, (su, sv) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
        side1 = (m >> np.uint32(_offset_bit({a: front, u: su}))) & np.uint32(1)
        side2 = (m >> np.uint32(_offset_bit({a: front, v: sv}))) & np.uint32(1)
        corner = (m >> np.uint32(_offset_bit({a: front, u: su, v: sv}))) & np.uint32(1)
        out[..., k] = np.where((side1 & side2) != 0, 0, 3 - (side1 + side2 + corner)).astype(np.uint8)
    return out


class VoxelVolume:
    """Device-resident editable occupancy of an S^3 volume (include/vrc.h: vrc_volume_*).  Edits are batched; commit()
    builds a new immutable LSVO on the device, bit-identical to compileSVO of the current voxel set."""

    def __init__(self, depth, device=0):
        self._h = C.c_void_p()
        check(capi.load().vrc_volume_create(depth, device, C.byref(self._h)))
        self.depth, self.device = depth, device

    @classmethod
    def fromScene(cls, svo):
        """Rasterise a resident scene (e.g. LSVO.fromFastNoiseTerrain) into a volume; takes over its albedo tables."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        check(capi.load().vrc_volume_from_scene(svo._h, C.byref(self._h)))
        self.depth, self.device = svo.depth, svo.device
        return self

    def setVoxels(self, xyz, solid=True):
        """xyz: (n, 3) voxel coordinates, all set or all cleared; out-of-volume ones are dropped.  Synchronous."""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        check(capi.load().vrc_volume_set_voxels(self._h, xyz.shape[0], ptr(xyz), int(bool(solid)), capi.VRC_MEM_HOST, None))

    def setVoxelsDevice(self, n, xyz_ptr, solid=True, stream=None):
        """the same over n x 3 uint32 in device memory, asynchronous on `stream`"""
        check(capi.load().vrc_volume_set_voxels(self._h, n, ptr(xyz_ptr), int(bool(solid)), capi.VRC_MEM_DEVICE, ptr(stream)))

    def fillBoxes(self, lo_hi, solid=True):
        """lo_hi: (n, 6) = lo x y z (inclusive), hi x y z (exclusive); clipped to the volume.  Synchronous."""
        lo_hi = np.ascontiguousarray(lo_hi, np.uint32).reshape(-1, 6)
        check(capi.load().vrc_volume_fill_boxes(self._h, lo_hi.shape[0], ptr(lo_hi), int(bool(solid)), capi.VRC_MEM_HOST, None))

    def fillBoxesDevice(self, n, lo_hi_ptr, solid=True, stream=None):
        check(capi.load().vrc_volume_fill_boxes(self._h, n, ptr(lo_hi_ptr), int(bool(solid)), capi.VRC_MEM_DEVICE, ptr(stream)))

    def fillSpheres(self, centre_radius, solid=True):
        """centre_radius: (n, 4) int32 = centre x y z (signed, may lie outside), radius; the voxels with
        dx^2 + dy^2 + dz^2 <= r^2 are set or cleared.  Synchronous."""
        cr = np.ascontiguousarray(centre_radius, np.int32).reshape(-1, 4)
        check(capi.load().vrc_volume_fill_spheres(self._h, cr.shape[0], ptr(cr), int(bool(solid)), capi.VRC_MEM_HOST, None))

    def fillSpheresDevice(self, n, centre_radius_ptr, solid=True, stream=None):
        check(capi.load().vrc_volume_fill_spheres(self._h, n, ptr(centre_radius_ptr), int(bool(solid)), capi.VRC_MEM_DEVICE, ptr(stream)))

    def fillSpheresAtHits(self, hits, radius, solid=True):
        """One sphere at every castRays record: solid=False digs at the voxel hit, solid=True builds at the empty cell the
        ray came through; misses, LOD cut-offs and records without such a cell are skipped.  Synchronous."""
        hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
        check(capi.load().vrc_volume_fill_spheres_at_hits(self._h, hits.shape[0], ptr(hits), int(radius), int(bool(solid)), capi.VRC_MEM_HOST, None))

    def fillSpheresAtHitsDevice(self, n, hits_ptr, radius, solid=True, stream=None):
        """the same over the records castRaysDevice left in device memory; on the same stream no host copy and no
        synchronisation lies between the cast and the edit"""
        check(capi.load().vrc_volume_fill_spheres_at_hits(self._h, n, ptr(hits_ptr), int(radius), int(bool(solid)), capi.VRC_MEM_DEVICE, ptr(stream)))

    def fillCapsules(self, items, solid=True):
        """items: (n, 8) int32 = a x y z, b x y z, radius, 0 (signed, may lie outside): the voxels within `radius` of the
        segment a-b, by the exact integer rule of include/vrc.h (vrc_stroke_fill_capsules), are set or cleared.  Synchronous."""
        items = np.ascontiguousarray(items, np.int32).reshape(-1, 8)
        check(capi.load().vrc_stroke_fill_capsules(self._h, items.shape[0], ptr(items), int(bool(solid)), capi.VRC_MEM_HOST, None))

    def fillCapsulesDevice(self, n, items_ptr, solid=True, stream=None):
        check(capi.load().vrc_stroke_fill_capsules(self._h, n, ptr(items_ptr), int(bool(solid)), capi.VRC_MEM_DEVICE, ptr(stream)))

    def strokeAtHits(self, hits, radius, solid=True, max_gap=0):
        """The gapless stroke through castRays records: the centres of fillSpheresAtHits, each joined to the next by a capsule
        of `radius`; a record without a centre breaks the stroke, and so does a step of more than max_gap voxels (0: no
        limit).  Synchronous."""
        hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
        check(capi.load().vrc_stroke_fill_at_hits(self._h, hits.shape[0], ptr(hits), int(radius), int(max_gap), int(bool(solid)),
                                                  capi.VRC_MEM_HOST, None))

    def strokeAtHitsDevice(self, n, hits_ptr, radius, solid=True, max_gap=0, stream=None):
        """the same over the records castRaysDevice left in device memory, on the same stream with no host copy"""
        check(capi.load().vrc_stroke_fill_at_hits(self._h, n, ptr(hits_ptr), int(radius), int(max_gap), int(bool(solid)),
                                                  capi.VRC_MEM_DEVICE, ptr(stream)))

    def fillLine(self, a, b, r=0, solid=True):
        """one capsule from voxel a to voxel b; r = 0 is the lattice points on the segment"""
        self.fillCapsules([tuple(a) + tuple(b) + (r, 0)], solid)

    def fillPolyline(self, points, r=0, solid=True, closed=False):
        """one capsule per pair of successive points (and from the last back to the first when closed), in one call; a single
        point is its ball"""
        pts = np.asarray(points, np.int64).reshape(-1, 3)
        if len(pts) == 0:
            return
        if len(pts) == 1:
            first = nxt = pts
        elif closed:
            first, nxt = pts, np.roll(pts, -1, axis=0)
        else:
            first, nxt = pts[:-1], pts[1:]
        items = np.zeros((len(first), 8), np.int32)
        items[:, 0:3], items[:, 3:6], items[:, 6] = first, nxt, r
        self.fillCapsules(items, solid)

    def copyRegion(self, src, src_lo, size, dst_lo, op=capi.VRC_COPY_REPLACE, stream=None):
        """Voxels src_lo + d of the volume `src` (any depth, same device) go to dst_lo + d of this one for 0 <= d < size,
        clipped to both; op = capi.VRC_COPY_REPLACE / _OR / _ANDNOT.  Asynchronous on `stream`."""
        src_lo = np.ascontiguousarray(src_lo, np.uint32).reshape(3)
        size = np.ascontiguousarray(size, np.uint32).reshape(3)
        dst_lo = np.ascontiguousarray(dst_lo, np.int32).reshape(3)
        check(capi.load().vrc_volume_copy_region(self._h, src._h, ptr(src_lo), ptr(size), ptr(dst_lo), int(op), ptr(stream)))

    def stampAffine(self, src, affine, dst_lo=None, dst_hi=None, op=capi.VRC_COPY_REPLACE, stream=None):
        """Stamps the volume `src` (any depth, same device) into this one through the inverse map `affine` (a capi.Affine,
        e.g. from affine_signed_permutation / affine_place / make_affine): every voxel p of the box [dst_lo, dst_hi) -- the
        whole volume by default -- takes (op) the source voxel (m (2p + 1) + t) >> 17, empty where that lies outside src
        (include/vrc.h: vrc_volume_stamp_affine).  Asynchronous on `stream`."""
        size = 1 << self.depth
        lo = np.ascontiguousarray((0, 0, 0) if dst_lo is None else dst_lo, np.uint32).reshape(3)
        hi = np.ascontiguousarray((size, size, size) if dst_hi is None else dst_hi, np.uint32).reshape(3)
        check(capi.load().vrc_volume_stamp_affine(self._h, src._h, C.byref(affine), ptr(lo), ptr(hi), int(op), ptr(stream)))

    def stampPlaced(self, src, rot, scale=1.0, src_pivot=None, dst_pivot=None, op=capi.VRC_COPY_OR, stream=None):
        """Places `src` in this volume turned by rot (make_rotation's layout) and resized by scale about the pivots
        (continuous voxel coordinates; the two volumes' centres by default): affine_place, then stampAffine of the box it
        names.  Returns (affine, lo, hi)."""
        if src_pivot is None:
            src_pivot = (float(1 << (src.depth - 1)),) * 3
        if dst_pivot is None:
            dst_pivot = (float(1 << (self.depth - 1)),) * 3
        affine, lo, hi = affine_place(rot, scale, src_pivot, dst_pivot, src.depth, self.depth)
        self.stampAffine(src, affine, lo, hi, op, stream)
        return affine, lo, hi

    def transformed(self, affine, depth=None):
        """A new volume of `depth` (this one's by default) on the same device that holds the stamp of this volume through
        `affine`: affine_signed_permutation((1, 0, 2), (0, 1, 0), S) turns a clipboard a quarter turn."""
        out = VoxelVolume(self.depth if depth is None else depth, self.device)
        try:
            out.stampAffine(self, affine)
        except Exception:
            out.close()
            raise
        return out

    def clone(self):
        """A new volume with this one's occupancy (after every edit issued so far) and albedo tables: the undo snapshot."""
        other = VoxelVolume.__new__(VoxelVolume)
        other._h = C.c_void_p()
        check(capi.load().vrc_volume_clone(self._h, C.byref(other._h)))
        other.depth, other.device = self.depth, self.device
        return other

    def diff(self, after):
        """What changed from this volume to `after` (same depth and device), as a VoxelDelta: one record per occupancy word
        that differs (include/vrc.h: vrc_delta_diff).  Both volumes are only read.  Synchronous."""
        handle, stats = C.c_void_p(), capi.DeltaStats()
        check(capi.load().vrc_delta_diff(self._h, after._h, C.byref(handle), C.byref(stats)))
        return VoxelDelta(handle, stats, self.depth, self.device)

    def applyDelta(self, delta, stream=None):
        """word ^= bits for every record of the delta: on the `before` of a diff it gives `after`, on `after` it gives
        `before` (undo and redo are one call), on an empty volume the set of changed voxels.  Asynchronous on `stream`."""
        check(capi.load().vrc_delta_apply(delta._h, self._h, ptr(stream)))

    def deltaFromRecords(self, records):
        """a VoxelDelta for this volume's depth and device from caller records (VoxelDelta.fromRecords)"""
        return VoxelDelta.fromRecords(self.depth, records, self.device)

    def deltaFromRecordsDevice(self, n, records_ptr):
        return VoxelDelta.fromRecordsDevice(self.depth, n, records_ptr, self.device)

    countMask = staticmethod(count_mask)

    def cellStep(self, birth, survive, neighbours=26, outside=False, dst=None, count_changed=False, stream=None):
        """One step of the neighbour-count automaton (include/vrc.h: vrc_cells_step): with c the number of solid voxels among
        a voxel's 6 or 26 neighbours (those beyond the faces solid with `outside`), a solid voxel stays if bit c of `survive`
        is set and an empty one becomes solid if bit c of `birth` is; both are bit masks or iterables of counts.  This
        volume is only read; the result is written whole into `dst`, a new volume by default.  Returns dst -- or, with
        count_changed, (dst, the number of voxels that differ), which makes the call synchronous; else it is asynchronous on
        `stream`."""
        made = dst is None
        if made:
            dst = VoxelVolume(self.depth, self.device)
        changed = C.c_uint64()
        try:
            check(capi.load().vrc_cells_step(dst._h, self._h, int(neighbours), self.countMask(birth), self.countMask(survive), int(outside),
                                             C.cast(C.byref(changed), C.c_void_p) if count_changed else None, capi.VRC_MEM_HOST, ptr(stream)))
        except Exception:
            if made:
                dst.close()
            raise
        return (dst, int(changed.value)) if count_changed else dst

    def cellStepDevice(self, dst, birth, survive, changed_ptr, neighbours=26, outside=False, stream=None):
        """the same with the count in one device uint64 (or None), zeroed and written in stream order: asynchronous"""
        check(capi.load().vrc_cells_step(dst._h, self._h, int(neighbours), self.countMask(birth), self.countMask(survive), int(outside),
                                         ptr(changed_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def automaton(self, steps, birth, survive, neighbours=26, outside=False):
        """Up to `steps` steps of cellStep in place, ping-pong with one scratch volume that lives for the call.  It ends
        early at a fixed point, a step that changes nothing; the result is left in this volume.  Returns the steps taken:
        the number of steps that changed a voxel, at most `steps`."""
        taken = 0
        if steps <= 0:
            return taken
        src, dst = self, VoxelVolume(self.depth, self.device)
        scratch = dst
        try:
            while taken < steps:
                _, changed = src.cellStep(birth, survive, neighbours, outside, dst, count_changed=True)
                if not changed:
                    break                                     # dst equals src: whichever of the two this volume is, it holds the result
                src, dst = dst, src
                taken += 1
            if src is not self and taken:
                size = 1 << self.depth
                self.copyRegion(src, (0, 0, 0), (size, size, size), (0, 0, 0))
        finally:
            scratch.close()                                   # waits for the copy
        return taken

    def smooth(self, iterations=1, outside=False):
        """The majority vote of the 27 cells around every voxel, itself included, `iterations` times in place (ending early
        at a fixed point): solid where at least 14 of the 27 are.  Rounds a voxelised model, fills pin-holes, removes
        specks.  With `outside` everything beyond the faces votes solid."""
        self.automaton(iterations, range(14, 27), range(13, 27), capi.VRC_CELLS_ALL, outside)
        return self

    def removeSpecks(self):
        """Clears every solid voxel none of whose six face neighbours is solid (the faces of the volume are empty); in place"""
        self.automaton(1, 0, range(1, 7), capi.VRC_CELLS_FACES, False)
        return self

    def fillRandom(self, seed, density, box=None, op=capi.VRC_COPY_OR, stream=None):
        """A seeded random voxel set R (include/vrc.h: vrc_cells_fill_random): a hash of (seed, x, y, z) below
        round(density 2^32), the same field at every depth and in every box.  Inside `box` (lo x y z, hi x y z exclusive,
        clipped; the whole volume by default) the volume takes (op) R.  Asynchronous on `stream`."""
        if not 0.0 <= density <= 1.0:
            raise ValueError(f"fillRandom: density {density} not in [0, 1]")
        lo_hi = None if box is None else np.ascontiguousarray(box, np.uint32).reshape(6)
        check(capi.load().vrc_cells_fill_random(self._h, int(seed) & 0xFFFFFFFF, int(np.floor(density * 4294967296.0 + 0.5)), ptr(lo_hi), int(op), ptr(stream)))
        return self

    def caves(self, seed, density, steps):
        """Procedural caves in place: the random fill of the whole volume (REPLACE), then `steps` rounds of smooth with
        everything beyond the faces solid, so that the caves close towards the faces"""
        self.fillRandom(seed, density, None, capi.VRC_COPY_REPLACE)
        return self.smooth(steps, outside=True)

    def _rect(self, rect):
        """(the 4 uint32 of a rect or None, its shape (U, V))"""
        S = 1 << self.depth
        if rect is None:
            return None, (S, S)
        r = np.ascontiguousarray(rect, np.uint32).reshape(4)
        return r, (max(int(r[2]) - int(r[0]), 0), max(int(r[3]) - int(r[1]), 0))

    def columnProfile(self, direction, rect=None, device=False):
        """What every column holds, met along direction = 2 * axis + side (side 0 travels towards smaller coordinates, as for
        dropLoose): a (U, V) array of capi.COLUMN_DTYPE with the coordinate of the `first` and `last` solid voxel met
        (capi.VRC_COLUMN_NONE in an empty column), the `count` of solid voxels and the `runs` of consecutive ones (include/vrc.h:
        vrc_columns_profile).  (U, V) are the other two axes in x < y < z order; rect = (u_lo, v_lo, u_hi, v_hi), the whole
        face by default.  device: the records stay on the device, as a torch tensor of shape (U, V, 4) int32.  Synchronous."""
        r, shape = self._rect(rect)
        if device:
            import torch
            out = torch.empty(shape + (4,), dtype=torch.int32, device=f"cuda:{self.device}")
            check(capi.load().vrc_columns_profile(self._h, int(direction), ptr(r), ptr(out.data_ptr()), capi.VRC_MEM_DEVICE, None))
            check(capi.load().vrc_stream_synchronize(self.device, None))
            return out
        out = np.empty(shape, capi.COLUMN_DTYPE)
        check(capi.load().vrc_columns_profile(self._h, int(direction), ptr(r), ptr(out), capi.VRC_MEM_HOST, None))
        return out

    def columnProfileDevice(self, direction, out_ptr, rect=None, stream=None):
        """the same into U x V records of 16 bytes in device memory, asynchronous on `stream`"""
        check(capi.load().vrc_columns_profile(self._h, int(direction), ptr(self._rect(rect)[0]), ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def heightMap(self, direction, none=-1):
        """int32 (S, S): the coordinate of the first solid voxel met along `direction` in every column, `none` where there is
        none.  heightMap(2) is the top-down map of a y-up world."""
        p = self.columnProfile(direction)
        return np.where(p["count"] > 0, p["first"].astype(np.int64), none).astype(np.int32)

    def thicknessMap(self, axis):
        """uint32 (S, S): the solid voxels of every column along `axis`, the X-ray image; it sums to solidCount()"""
        return self.columnProfile(2 * int(axis))["count"].copy()

    def isHeightField(self, direction, grounded=False):
        """True if no column has a second run met along `direction`: no overhang and no cave under the surface that the
        direction sees.  grounded: every run must also reach the exit face."""
        p = self.columnProfile(direction)
        exit_at = (1 << self.depth) - 1 if int(direction) & 1 else 0
        return bool((p["runs"] <= 1).all() and (not grounded or (p["last"][p["runs"] == 1] == exit_at).all()))

    def fillColumns(self, axis, lo, hi, rect=None, op=capi.VRC_COPY_OR, stream=None):
        """Every column of the rect takes (op) its span [lo, hi) along `axis` (include/vrc.h: vrc_columns_fill): lo and hi are
        integers or int32 maps of the rect's shape (U, V), clamped to [0, S]; under capi.VRC_COPY_REPLACE the rest of the
        column is cleared.  Synchronous when a map is given, else asynchronous on `stream`."""
        r, shape = self._rect(rect)
        maps, consts = [], []
        for bound in (lo, hi):
            if np.ndim(bound) == 0:
                maps.append(None)
                consts.append(int(max(-(1 << 31), min((1 << 31) - 1, int(bound)))))
            else:
                m = np.ascontiguousarray(bound, np.int32)
                if m.shape != shape:
                    raise ValueError(f"fillColumns: a map of shape {m.shape} for a rect of {shape}")
                maps.append(m)
                consts.append(0)
        mem = capi.VRC_MEM_DEVICE if maps[0] is None and maps[1] is None else capi.VRC_MEM_HOST
        check(capi.load().vrc_columns_fill(self._h, int(axis), ptr(r), ptr(maps[0]), consts[0], ptr(maps[1]), consts[1], int(op), mem, ptr(stream)))
        return self

    def fillColumnsDevice(self, axis, lo_ptr, lo_const, hi_ptr, hi_const, rect=None, op=capi.VRC_COPY_OR, stream=None):
        """the same with the maps (or None) in device memory, asynchronous on `stream`"""
        check(capi.load().vrc_columns_fill(self._h, int(axis), ptr(self._rect(rect)[0]), ptr(lo_ptr), int(lo_const), ptr(hi_ptr), int(hi_const), int(op),
                                           capi.VRC_MEM_DEVICE, ptr(stream)))
        return self

    def raiseTerrain(self, heights):
        """The reference's terrain rule (main.cpp:65-72) as an editable volume: column (x, z) becomes solid for
        S/2 + 1 <= y < S/2 + clamp(heights[x, z], 16, S), everything else is cleared.  Committed, it is the scene that
        LSVO.fromTerrain builds from the same heights."""
        S = 1 << self.depth
        h = np.asarray(heights)[:S, :S]
        if h.shape != (S, S):
            raise ValueError(f"raiseTerrain: heights of shape {np.asarray(heights).shape} for a volume of {S}")
        hi = S // 2 + np.clip(h.astype(np.int64), 16, S)
        return self.fillColumns(1, S // 2 + 1, hi.astype(np.int32), None, capi.VRC_COPY_REPLACE)

    def selectColumns(self, direction, lo, hi, of, dst=None, op=capi.VRC_COPY_REPLACE, stream=None):
        """dst (a new volume with None) takes (op) the voxels with lo <= P < hi, P the solid voxels met before the voxel along
        `direction`, that are solid (of = capi.VRC_COLUMNS_SOLID), empty (capi.VRC_COLUMNS_EMPTY) or either (3) (include/vrc.h:
        vrc_columns_select).  This volume is only read.  Asynchronous on `stream`; returns dst."""
        made = dst is None
        if made:
            dst = VoxelVolume(self.depth, self.device)
        try:
            check(capi.load().vrc_columns_select(dst._h, self._h, int(direction), int(lo), int(hi), int(of), int(op), ptr(stream)))
        except Exception:
            if made:
                dst.close()
            raise
        return dst

    def skyLit(self, direction):
        """a new volume: the solid voxels a parallel light along `direction` reaches, one per non-empty column"""
        return self.selectColumns(direction, 0, 1, capi.VRC_COLUMNS_SOLID)

    def topLayers(self, direction, k):
        """a new volume: the first k solid voxels of every column met along `direction`, the topsoil"""
        return self.selectColumns(direction, 0, int(k), capi.VRC_COLUMNS_SOLID)

    def sheltered(self, direction):
        """a new volume: the empty voxels behind a solid one along `direction`, overhangs and caves alike"""
        return self.selectColumns(direction, 1, (1 << self.depth) + 1, capi.VRC_COLUMNS_EMPTY)

    countRange = staticmethod(count_range)

    def cellCounts(self, k, device=False):
        """The density grid: uint32 (Sc, Sc, Sc) with Sc = S >> k, the number of solid voxels in every cube of 2^k voxels per
        axis, 1 <= k <= depth (include/vrc.h: vrc_levels_counts); cellCounts(depth)[0, 0, 0] is solidCount().  device: the counts
        stay on the device, as a torch tensor of dtype int32 (the same bits).  Synchronous."""
        sc = 1 << max(self.depth - int(k), 0)
        if device:
            import torch
            out = torch.empty((sc, sc, sc), dtype=torch.int32, device=f"cuda:{self.device}")
            check(capi.load().vrc_levels_counts(self._h, int(k), ptr(out.data_ptr()), capi.VRC_MEM_DEVICE, None))
            check(capi.load().vrc_stream_synchronize(self.device, None))
            return out
        out = np.empty((sc, sc, sc), np.uint32)
        check(capi.load().vrc_levels_counts(self._h, int(k), ptr(out), capi.VRC_MEM_HOST, None))
        return out

    def cellCountsDevice(self, k, out_ptr, stream=None):
        """the same into (S >> k)^3 uint32 in device memory, asynchronous on `stream`"""
        check(capi.load().vrc_levels_counts(self._h, int(k), ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def reduceInto(self, dst, lo, hi, op=capi.VRC_COPY_REPLACE, stream=None):
        """The volume `dst` of a smaller depth (same device) takes (op) the voxels whose cell of this volume -- the cube of 2^k
        voxels per axis, k the difference of the depths -- holds lo <= count < hi solid voxels (include/vrc.h:
        vrc_levels_reduce; count_range names the usual bands).  This volume is only read.  Asynchronous on `stream`; returns
        dst."""
        check(capi.load().vrc_levels_reduce(dst._h, self._h, min(int(lo), 0xFFFFFFFF), min(int(hi), 0xFFFFFFFF), int(op), ptr(stream)))
        return dst

    def expandInto(self, dst, op=capi.VRC_COPY_REPLACE, stream=None):
        """The volume `dst` of a greater depth (same device) takes (op) this volume with every voxel repeated 2^k times per
        axis: voxel p of dst is voxel p >> k of this one (include/vrc.h: vrc_levels_expand).  Asynchronous on `stream`; returns
        dst."""
        check(capi.load().vrc_levels_expand(dst._h, self._h, int(op), ptr(stream)))
        return dst

    def _made(self, depth, fill):
        out = VoxelVolume(int(depth), self.device)
        try:
            fill(out)
        except Exception:
            out.close()
            raise
        return out

    def reduced(self, depth, rule="any"):
        """a new volume of the smaller `depth`: reduceInto with the band of count_range(rule, self.depth - depth) -- "any" is the
        conservative proxy, "all" the interior, "majority" keeps the volume, or a pair (lo, hi)"""
        lo, hi = count_range(rule, self.depth - int(depth))
        return self._made(depth, lambda out: self.reduceInto(out, lo, hi))

    def expanded(self, depth):
        """a new volume of the greater `depth` that holds this one blown up"""
        return self._made(depth, lambda out: self.expandInto(out))

    def levels(self, rule="any"):
        """the reductions of this volume to every depth from depth - 1 down to 2, finest first, each reduced directly from this
        volume: count thresholds do not compose from level to level"""
        out = []
        try:
            for depth in range(self.depth - 1, 1, -1):
                out.append(self.reduced(depth, rule))
        except Exception:
            for v in out:
                v.close()
            raise
        return out

    def getVoxels(self, xyz):
        """uint8 0 / 1 per (n, 3) voxel coordinate, 0 outside the volume.  Synchronous."""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        out = np.zeros(xyz.shape[0], np.uint8)
        check(capi.load().vrc_volume_get_voxels(self._h, xyz.shape[0], ptr(xyz), ptr(out), capi.VRC_MEM_HOST, None))
        return out

    def getVoxelsDevice(self, n, xyz_ptr, solid_out_ptr, stream=None):
        check(capi.load().vrc_volume_get_voxels(self._h, n, ptr(xyz_ptr), ptr(solid_out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def countBoxes(self, lo_hi):
        """solid voxels per (n, 6) box (lo inclusive, hi exclusive, clipped to the volume), uint64.  Synchronous."""
        lo_hi = np.ascontiguousarray(lo_hi, np.uint32).reshape(-1, 6)
        out = np.zeros(lo_hi.shape[0], np.uint64)
        check(capi.load().vrc_volume_count_boxes(self._h, lo_hi.shape[0], ptr(lo_hi), ptr(out), capi.VRC_MEM_HOST, None))
        return out

    def countBoxesDevice(self, n, lo_hi_ptr, counts_ptr, stream=None):
        check(capi.load().vrc_volume_count_boxes(self._h, n, ptr(lo_hi_ptr), ptr(counts_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def flood(self, medium, connectivity=6, through_empty=False, max_sweeps=0):
        """Flood fill by connectivity (include/vrc.h: vrc_volume_flood): this volume's solid voxels are the seeds; afterwards
        it holds exactly the voxels of `medium` (its solid ones, or its empty ones with through_empty) joined to a seed by
        face neighbours (connectivity=6) or face / edge / corner neighbours (26).  max_sweeps=0 runs to convergence; a capped
        call may return converged == 0 with a valid partial result, and calling again continues.  Synchronous.  Returns
        capi.FloodStats (reached, sweeps, converged)."""
        st = capi.FloodStats()
        check(capi.load().vrc_volume_flood(self._h, medium._h, int(connectivity), capi.VRC_FLOOD_EMPTY if through_empty else capi.VRC_FLOOD_SOLID,
                                           int(max_sweeps), C.byref(st)))
        return st

    def keepConnected(self, anchor_boxes, connectivity=6):
        """Drops what no longer holds on to the anchors: afterwards this volume holds only the solid voxels joined to a
        solid voxel inside one of the (n, 6) anchor boxes, and the rest -- the debris -- is returned as a new volume."""
        S = 1 << self.depth
        whole = ((0, 0, 0), (S, S, S), (0, 0, 0))
        supported = VoxelVolume(self.depth, self.device)
        supported.fillBoxes(anchor_boxes)
        supported.flood(self, connectivity)
        debris = self.clone()
        debris.copyRegion(supported, *whole, op=capi.VRC_COPY_ANDNOT)
        self.copyRegion(supported, *whole, op=capi.VRC_COPY_REPLACE)
        # the copies run on the NULL stream; `supported` is destroyed behind them (vrc_volume_destroy waits for the device)
        supported.close()
        return debris

    def dropLoose(self, anchor_boxes, direction, connectivity=6, drop_limit=0):
        """Dig, let the debris fall, commit: what no longer holds on to a solid voxel inside one of the (n, 6) anchor boxes
        (keepConnected) falls piece by piece as rigid bodies along `direction` (a capi.VRC_FACE_* code, no default: on the
        terrain generator's scenes the ground lies towards -y, capi.VRC_FACE_YN) until it lands on the supported part, on
        another piece or on the volume's face, at most drop_limit cells (0 = no limit) -- include/vrc.h: vrc_fall_drops.
        Afterwards the volume holds the supported part plus every loose piece where it came to rest.  Returns capi.FallStats."""
        debris = self.keepConnected(anchor_boxes, connectivity)
        try:
            labels = debris.labelComponents(connectivity)
            try:
                offsets, stats = labels.fall(self, direction, drop_limit)
                labels.place(offsets, self, capi.VRC_COPY_OR)
            finally:
                labels.close()
        finally:
            debris.close()
        return stats

    def labelComponents(self, connectivity=6, through_empty=False):
        """Every connected piece of the solid voxels (or, with through_empty, of the empty ones) named in one call
        (include/vrc.h: vrc_volume_label_components): a VoxelLabels snapshot that later edits do not change.  Synchronous."""
        handle, count = C.c_void_p(), C.c_uint64()
        check(capi.load().vrc_volume_label_components(self._h, int(connectivity), capi.VRC_FLOOD_EMPTY if through_empty else capi.VRC_FLOOD_SOLID,
                                                      C.byref(handle), C.byref(count)))
        return VoxelLabels(handle, int(count.value), self.depth, self.device)

    def fracture(self, sites, connectivity=6, through_empty=False, max_distance=None):
        """Voronoi fracture (include/vrc.h: vrc_fracture_label): the pieces of the solid voxels (or, with through_empty, of the
        empty ones) cut along the Voronoi cells of the (n, 3) int32 `sites` -- every voxel belongs to its nearest in-volume
        site, among several nearest to the lowest index; voxels farther than max_distance from every site (d^2 > r^2, the
        radius rule of fillSpheres; None: no limit) keep the cell "none" and stay whole.  Nothing is removed.  A VoxelLabels
        snapshot whose pieceSites() names each piece's cell.  Synchronous."""
        sites = np.ascontiguousarray(sites, np.int32).reshape(-1, 3)
        max_d2 = capi.VRC_DISTANCE_NONE if max_distance is None else self._radius(max_distance, "fracture") ** 2
        handle, count = C.c_void_p(), C.c_uint64()
        check(capi.load().vrc_fracture_label(self._h, int(connectivity), capi.VRC_FLOOD_EMPTY if through_empty else capi.VRC_FLOOD_SOLID, sites.shape[0],
                                             ptr(sites) if sites.shape[0] else None, max_d2, capi.VRC_MEM_HOST, C.byref(handle), C.byref(count)))
        return VoxelLabels(handle, int(count.value), self.depth, self.device)

    def fractureDevice(self, n, sites_ptr, connectivity=6, through_empty=False, max_distance=None):
        """the same over n x 3 int32 sites in device memory; still synchronous"""
        max_d2 = capi.VRC_DISTANCE_NONE if max_distance is None else self._radius(max_distance, "fractureDevice") ** 2
        handle, count = C.c_void_p(), C.c_uint64()
        check(capi.load().vrc_fracture_label(self._h, int(connectivity), capi.VRC_FLOOD_EMPTY if through_empty else capi.VRC_FLOOD_SOLID, n, ptr(sites_ptr),
                                             max_d2, capi.VRC_MEM_DEVICE, C.byref(handle), C.byref(count)))
        return VoxelLabels(handle, int(count.value), self.depth, self.device)

    def shatter(self, sites, max_distance, direction, connectivity=6, drop_limit=0):
        """Break, let the shards fall, ready to commit: the solid within max_distance of the `sites` is cut into Voronoi shards
        (fracture), the shards -- the pieces whose cell is a site -- are taken out of the volume, fall as rigid bodies along
        `direction` (a capi.VRC_FACE_* code) onto what is left, onto each other or onto the volume's face, at most drop_limit
        cells (0 = no limit), and are put back where they come to rest.  Returns (capi.FallStats, the VoxelLabels).  The labels
        are what a physics engine goes on with: poses() for tumbling shards, contacts() against the world, and
        candidatePairs() / pairContacts() for shard against shard."""
        labels = self.fracture(sites, connectivity, False, max_distance)
        try:
            shards = (labels.pieceSites() != capi.VRC_NO_COMPONENT).astype(np.uint8)
            labels.select(shards, self, capi.VRC_COPY_ANDNOT)
            offsets, stats = labels.fall(self, direction, drop_limit)
            labels.place(offsets, self, capi.VRC_COPY_OR, keep=shards)
        except Exception:
            labels.close()
            raise
        return stats, labels

    def removeSmallPieces(self, min_voxels, connectivity=6):
        """Clears every solid piece of fewer than min_voxels voxels (the specks a dig or a leaky mesh leaves); returns
        (pieces before, pieces removed)."""
        labels = self.labelComponents(connectivity)
        small = (labels.components()["voxels"] < min_voxels).astype(np.uint8)
        if small.any():
            labels.select(small, self, capi.VRC_COPY_ANDNOT)
        labels.close()
        return len(small), int(small.sum())

    def splitPieces(self, connectivity=6, max_pieces=None):
        """The solid pieces as bodies: (records in id order, [(id, VoxelVolume holding that piece alone), ...]) for the
        max_pieces largest pieces (all of them with None), largest first, ties by id."""
        labels = self.labelComponents(connectivity)
        records = labels.components()
        order = np.argsort(-records["voxels"].astype(np.int64), kind="stable")
        if max_pieces is not None:
            order = order[:max_pieces]
        pieces = []
        for i in order:
            keep = np.zeros(len(records), np.uint8)
            keep[i] = 1
            pieces.append((int(i), labels.select(keep)))
        labels.close()
        return records, pieces

    def distanceField(self, to_empty=False, outside=False):
        """The exact squared Euclidean distance of every voxel to the nearest solid voxel (to the nearest empty one with
        to_empty; with outside, everything beyond the volume's faces counts as a feature too) -- include/vrc.h:
        vrc_volume_distance_field.  A VoxelDistance snapshot that later edits do not change.  Synchronous."""
        handle, stats = C.c_void_p(), capi.DistanceStats()
        check(capi.load().vrc_volume_distance_field(self._h, capi.VRC_FLOOD_EMPTY if to_empty else capi.VRC_FLOOD_SOLID, int(bool(outside)),
                                                    C.byref(handle), C.byref(stats)))
        return VoxelDistance(handle, stats, self.depth, self.device)

    def travelField(self, seeds, connectivity=6, through_empty=False, step_limit=0):
        """The least number of steps from the solid voxels of the volume `seeds` to every voxel through this volume's solid
        voxels (its empty ones with through_empty), a step to a face neighbour (connectivity=6) or to a face / edge / corner
        neighbour (26) costing 1 -- include/vrc.h: vrc_travel_field.  capi.VRC_DISTANCE_NONE where nothing arrives
        and, with step_limit, beyond step_limit steps.  A VoxelDistance snapshot with `stats` a capi.TravelStats and
        `connectivity` 6 or 26; `seeds` may be this volume.  Synchronous."""
        handle, stats = C.c_void_p(), capi.TravelStats()
        check(capi.load().vrc_travel_field(seeds._h, self._h, int(connectivity), capi.VRC_FLOOD_EMPTY if through_empty else capi.VRC_FLOOD_SOLID,
                                                  int(step_limit), C.byref(handle), C.byref(stats)))
        return VoxelDistance(handle, stats, self.depth, self.device)

    def reachableWithin(self, seeds, steps, connectivity=6, through_empty=False):
        """A new volume holding the voxels that `steps` steps or fewer from `seeds` reach through this one (travelField
        with step_limit, then select)."""
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"reachableWithin: negative step count {steps}")
        if steps == 0:                    # step_limit 0 would mean "no limit": the seeds themselves are what 0 steps reach
            field = self.travelField(seeds, connectivity, through_empty, 1)
        else:
            field = self.travelField(seeds, connectivity, through_empty, min(steps, capi.VRC_DISTANCE_NONE - 1))
        out = field.select(0, min(steps, capi.VRC_DISTANCE_NONE - 1))
        field.close()
        return out

    def shortestPath(self, a, b, connectivity=6, through_empty=True):
        """A shortest route from voxel a to voxel b through this volume's empty voxels (its solid ones with
        through_empty=False) as a (T + 1, 3) uint32 array that starts at a and ends at b, or None when there is none: the
        travel field seeded at b, traced from a."""
        target = VoxelVolume(self.depth, self.device)
        try:
            target.setVoxels(np.asarray(b, np.uint32).reshape(1, 3))
            field = self.travelField(target, connectivity, through_empty)
        finally:
            target.close()
        try:
            lengths, paths = field.tracePaths(np.asarray(a, np.uint32).reshape(1, 3))
        finally:
            field.close()
        return None if lengths[0] == capi.VRC_DISTANCE_NONE else paths[0]

    def lineOfSight(self, a, b, radius=0):
        """Whether a ball of `radius` voxels (0: a thin ray) passes in a straight line from voxel a to voxel b without
        touching the solid: the distance field to the solid, then VoxelDistance.sight in supercover mode with lo =
        radius^2 + 1, the radius rule of fillSpheres.  False as well when an endpoint lies outside the volume.  For many
        segments keep the field and call its sight()."""
        r = self._radius(radius, "lineOfSight")
        field = self.distanceField()
        try:
            rec = field.sight(a, b, lo=r * r + 1, touch=True)
        finally:
            field.close()
        return bool(rec["status"][0] == capi.VRC_SIGHT_CLEAR)

    def visibleFrom(self, eye, radius=0):
        """A new volume holding the voxels an eye at voxel `eye` sees within `radius` voxels (0: no limit), the solid surface
        voxels at the end of a clear line included: the distance field to the solid, its sight field (VoxelDistance.visibleFrom)
        and a select of the finite values.  AND it with this volume for the visible blocks."""
        field = self.distanceField()
        try:
            seen = field.visibleFrom(eye, radius)
        finally:
            field.close()
        try:
            return seen.select(0, capi.VRC_DISTANCE_NONE - 1)
        finally:
            seen.close()

    @staticmethod
    def _radius(r, what):
        r = int(r)
        if r < 0:
            raise ValueError(f"{what}: negative radius {r}")
        return min(r, 65535)              # finite distances are below 2^22: every larger radius selects the same voxels

    def dilate(self, r):
        """Grows the solid set by r voxels in place: every voxel within d^2 <= r^2 of a solid one becomes solid (a
        fillSpheres of radius r at every solid voxel)."""
        r = self._radius(r, "dilate")
        field = self.distanceField()
        field.select(0, r * r, self, capi.VRC_COPY_OR)
        field.close()
        return self

    def erode(self, r, open_border=False):
        """Shrinks the solid set by r voxels in place: every voxel within d^2 <= r^2 of an empty one is cleared.  With
        open_border everything beyond the volume's faces counts as empty, so the erosion eats from the faces as well."""
        r = self._radius(r, "erode")
        field = self.distanceField(to_empty=True, outside=open_border)
        field.select(0, r * r, self, capi.VRC_COPY_ANDNOT)
        field.close()
        return self

    def openShape(self, r):
        """erode(r) then dilate(r): removes specks and sheets thinner than the ball, keeps the rest's outline"""
        r = self._radius(r, "openShape")
        return self.erode(r).dilate(r)

    def closeShape(self, r):
        """dilate(r) then erode(r) with the faces as walls: fills holes and gaps narrower than the ball"""
        r = self._radius(r, "closeShape")
        return self.dilate(r).erode(r, open_border=False)

    def hollow(self, t):
        """Clears every solid voxel farther than t from the empty voxels (D_empty > t^2), which leaves a shell t voxels
        thick; the faces of the volume are walls.  hollow(0) empties the volume."""
        t = self._radius(t, "hollow")
        field = self.distanceField(to_empty=True)
        field.select(t * t + 1, capi.VRC_DISTANCE_NONE, self, capi.VRC_COPY_ANDNOT)
        field.close()
        return self

    # ---- morphology by a structuring element of the caller's choice (include/vrc.h: vrc_morph_apply) ----

    def morph(self, what, offsets, dst=None, of_empty=False, outside=False, op=capi.VRC_COPY_REPLACE, origin=None, stream=None):
        """dst (a new volume with None) takes (op) K = A (+) E for what = capi.VRC_MORPH_DILATE, the p with some p - e in A, or
        K = A (-) E for capi.VRC_MORPH_ERODE, the p with every p + e in A.  A is this volume's solid voxels (its empty ones with
        of_empty) and, with `outside`, everything beyond the faces; E is the (n, 3) int32 `offsets` minus `origin`, every
        component within +-16 (element_ball, element_box, element_cross, element_line, element_of make them).  This volume is
        only read.  Synchronous; returns dst."""
        e = _element(offsets)
        o = None if origin is None else np.ascontiguousarray(origin, np.int32).reshape(3)
        made = dst is None
        if made:
            dst = VoxelVolume(self.depth, self.device)
        try:
            check(capi.load().vrc_morph_apply(dst._h, self._h, int(what), capi.VRC_MORPH_EMPTY if of_empty else capi.VRC_MORPH_SOLID, e.shape[0], ptr(e), ptr(o),
                                              int(bool(outside)), int(op), capi.VRC_MEM_HOST, ptr(stream)))
        except Exception:
            if made:
                dst.close()
            raise
        return dst

    def morphDevice(self, dst, what, n, offsets_ptr, origin=None, of_empty=False, outside=False, op=capi.VRC_COPY_REPLACE, stream=None):
        """the same with n x 3 int32 in device memory, asynchronous on `stream`: a uint32 x y z list of extractVoxelsDevice goes in
        as it is, with `origin` as the pivot.  An offset out of reach is dropped.  Returns dst."""
        o = None if origin is None else np.ascontiguousarray(origin, np.int32).reshape(3)
        check(capi.load().vrc_morph_apply(dst._h, self._h, int(what), capi.VRC_MORPH_EMPTY if of_empty else capi.VRC_MORPH_SOLID, int(n), ptr(offsets_ptr), ptr(o),
                                          int(bool(outside)), int(op), capi.VRC_MEM_DEVICE, ptr(stream)))
        return dst

    def _morphInPlace(self, what, element, outside):
        scratch = self.morph(what, element, outside=outside)
        try:
            size = 1 << self.depth
            self.copyRegion(scratch, (0, 0, 0), (size, size, size), (0, 0, 0))
        finally:
            scratch.close()                                   # waits for the copy
        return self

    def dilateBy(self, element):
        """Grows the solid set by the element in place (through a scratch volume that lives for the call): a voxel becomes
        solid when p - e is solid for some e.  Minkowski sums compose, so a box is three line elements in a row --
        dilateBy(element_line(0, -4, 4)).dilateBy(element_line(1, -4, 4)).dilateBy(element_line(2, -4, 4)) is the 9 x 9 x 9 box with
        27 offsets for 729, the way to do large boxes cheaply."""
        return self._morphInPlace(capi.VRC_MORPH_DILATE, element, False)

    def erodeBy(self, element, open_border=False):
        """Shrinks the solid set by the element in place: a voxel stays when p + e is solid for every e.  With open_border
        everything beyond the faces counts as empty, so the erosion eats from the faces as well (as erode does)."""
        return self._morphInPlace(capi.VRC_MORPH_ERODE, element, not open_border)

    def openBy(self, element):
        """erodeBy then dilateBy: keeps exactly the voxels that some copy of the element inside the solid set covers"""
        return self.erodeBy(element).dilateBy(element)

    def closeBy(self, element):
        """dilateBy then erodeBy with the faces as walls: fills what no copy of the element in the empty set reaches"""
        return self.dilateBy(element).erodeBy(element)

    def fitsAt(self, element):
        """A new volume: the pivots at which the shape stands free of the solid voxels and inside the volume -- the empty set
        eroded by the element.  travelField through it (seeds and medium) is the shortest path of an agent of that shape."""
        return self.morph(capi.VRC_MORPH_ERODE, element, of_empty=True, outside=False)

    def match(self, solid_offsets, empty_offsets, outside=False):
        """Hit-or-miss, a new volume: the p with p + s solid for every s of solid_offsets and p + t empty for every t of
        empty_offsets; beyond the faces everything is solid with `outside`, else empty."""
        out = self.morph(capi.VRC_MORPH_ERODE, solid_offsets, outside=outside)
        try:
            self.morph(capi.VRC_MORPH_DILATE, reflect(empty_offsets), out, outside=outside, op=capi.VRC_COPY_ANDNOT)
        except Exception:
            out.close()
            raise
        return out

    def xorMesh(self, tris_fixed, device=False, stream=None):
        """Solid voxelisation by crossing parity (include/vrc.h: vrc_volume_xor_mesh): (n, 9) int32 triangles in setCell
        coordinates with 6 fractional bits (64 units per voxel, voxel centres at 64 c + 32); every voxel whose centre lies
        under an odd number of them is flipped.  A closed mesh in an empty volume gives its inside.  Synchronous; with
        device=True tris_fixed is (n, device pointer to n x 9 int32) and the call is asynchronous on `stream`."""
        if device:
            n, tris_ptr = tris_fixed
            check(capi.load().vrc_volume_xor_mesh(self._h, int(n), ptr(tris_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))
            return
        tris = np.ascontiguousarray(tris_fixed, np.int32).reshape(-1, 9)
        check(capi.load().vrc_volume_xor_mesh(self._h, tris.shape[0], ptr(tris), capi.VRC_MEM_HOST, None))

    def rasterMesh(self, tris_fixed, mode=capi.VRC_RASTER_TOUCHED, solid=True, device=False, stream=None):
        """Surface voxelisation (include/vrc.h: vrc_raster_mesh): (n, 9) int32 triangles in xorMesh's fixed point.
        mode capi.VRC_RASTER_TOUCHED selects every voxel whose closed cube meets a triangle, capi.VRC_RASTER_THIN the voxel
        that holds each crossing of a voxel-centre line; the selected voxels are all set or all cleared.  Synchronous; with
        device=True tris_fixed is (n, device pointer to n x 9 int32) and the call is asynchronous on `stream`."""
        if device:
            n, tris_ptr = tris_fixed
            check(capi.load().vrc_raster_mesh(self._h, int(n), ptr(tris_ptr), int(mode), int(bool(solid)), capi.VRC_MEM_DEVICE, ptr(stream)))
            return
        tris = np.ascontiguousarray(tris_fixed, np.int32).reshape(-1, 9)
        check(capi.load().vrc_raster_mesh(self._h, tris.shape[0], ptr(tris), int(mode), int(bool(solid)), capi.VRC_MEM_HOST, None))

    def shellMesh(self, verts, faces, thin=False, solid=True, scale=1.0, offset=(0.0, 0.0, 0.0)):
        """Sets (or clears) the voxels the indexed mesh touches (verts (n, 3) float in voxels, faces (m, 3) indices), or with
        thin=True its thin shell; the mesh need not be closed."""
        fixed = self.quantiseMesh(verts, scale, offset)
        self.rasterMesh(fixed[np.asarray(faces, np.int64).reshape(-1, 3)].reshape(-1, 9),
                        capi.VRC_RASTER_THIN if thin else capi.VRC_RASTER_TOUCHED, solid)

    def solidFromShell(self, verts, faces, scale=1.0, offset=(0.0, 0.0, 0.0)):
        """The robust solid voxelisation: ORs into this volume the thin shell of the mesh plus every voxel that a
        face-connected flood of the empty medium, started on the volume's six faces, does not reach around that shell.  A
        doubled triangle or a self-intersection changes nothing, where xorMesh inverts columns; a mesh with a hole lets the
        flood in and leaves its shell alone.  Composition only: rasterMesh, fillBoxes, flood, copyRegion."""
        S = 1 << self.depth
        whole = ((0, 0, 0), (S, S, S), (0, 0, 0))
        shell = VoxelVolume(self.depth, self.device)
        outside = VoxelVolume(self.depth, self.device)
        try:
            shell.shellMesh(verts, faces, True, True, scale, offset)
            outside.fillBoxes([(0, 0, 0, S, S, 1), (0, 0, S - 1, S, S, S), (0, 0, 0, S, 1, S), (0, S - 1, 0, S, S, S),
                               (0, 0, 0, 1, S, S), (S - 1, 0, 0, S, S, S)])
            outside.copyRegion(shell, *whole, op=capi.VRC_COPY_ANDNOT)      # seeds: the empty voxels of the six faces
            outside.flood(shell, 6, through_empty=True)
            # unreached plus shell = everything the flood did not reach: the complement of `outside`
            shell.fillBoxes([(0, 0, 0, S, S, S)])
            shell.copyRegion(outside, *whole, op=capi.VRC_COPY_ANDNOT)
            self.copyRegion(shell, *whole, op=capi.VRC_COPY_OR)
        finally:
            shell.close()           # vrc_volume_destroy waits for the copies
            outside.close()

    @staticmethod
    def quantiseMesh(verts, scale=1.0, offset=(0.0, 0.0, 0.0)):
        """(n, 3) float vertices -> int32 fixed point, rint((v * scale + offset) * 64) in float64.  Each VERTEX once: a
        vertex shared by several faces stays one point, so a closed mesh stays closed."""
        v = np.asarray(verts, np.float64).reshape(-1, 3) * float(scale) + np.asarray(offset, np.float64).reshape(1, 3)
        q = np.rint(v * float(1 << capi.VRC_MESH_FRAC_BITS))
        if not np.all(np.abs(q) <= float(1 << 17)):          # NaN fails too
            raise VrcError("quantiseMesh: a vertex lies beyond +-2048 voxels (vrc_volume_xor_mesh would drop its triangles)")
        return q.astype(np.int32)

    def voxelizeMesh(self, verts, faces, scale=1.0, offset=(0.0, 0.0, 0.0)):
        """XORs the solid of the indexed mesh (verts (n, 3) float in voxels, faces (m, 3) indices) into the volume."""
        fixed = self.quantiseMesh(verts, scale, offset)
        self.xorMesh(fixed[np.asarray(faces, np.int64).reshape(-1, 3)].reshape(-1, 9))

    def stampMesh(self, verts, faces, op=capi.VRC_COPY_OR, scale=1.0, offset=(0.0, 0.0, 0.0)):
        """What an editor does with a model: voxelises it into a clipboard volume of the smallest depth that holds its
        bounding box and copies that box into this volume with op (capi.VRC_COPY_OR pastes, _ANDNOT carves, _REPLACE
        overwrites the box).  Returns (lo, size) of the box in this volume's voxels."""
        fixed = self.quantiseMesh(verts, scale, offset).astype(np.int64)
        lo = fixed.min(axis=0) >> capi.VRC_MESH_FRAC_BITS
        size = np.maximum(-((-fixed.max(axis=0)) >> capi.VRC_MESH_FRAC_BITS) - lo, 1)
        depth = 2
        while (1 << depth) < size.max():
            depth += 1
        if depth > 10:
            raise VrcError("stampMesh: the mesh's bounding box exceeds 1024 voxels")
        clip = VoxelVolume(depth, self.device)
        try:
            local = (fixed - (lo << capi.VRC_MESH_FRAC_BITS)).astype(np.int32)      # whole voxels: the same triangles, moved
            clip.xorMesh(local[np.asarray(faces, np.int64).reshape(-1, 3)].reshape(-1, 9))
            self.copyRegion(clip, (0, 0, 0), size, lo, op)
        finally:
            clip.close()        # vrc_volume_destroy waits for the copy
        return tuple(int(q) for q in lo), tuple(int(q) for q in size)

    # ---- getting the world out: the exposed faces as a mesh (include/vrc.h: vrc_volume_extract_surface) ----

    SURFACE_WINDOW = 1 << 20        # faces per call of the host forms with capacity=None

    def surfaceCount(self, closed=True):
        """(6,) uint64: exposed faces per direction d = 2 * axis + side (capi.VRC_FACE_*); closed=False leaves out the
        faces on the volume's own faces.  Synchronous."""
        out = np.zeros(6, np.uint64)
        check(capi.load().vrc_volume_surface_count(self._h, int(bool(closed)), ptr(out)))
        return out

    def _surface(self, fmt, dtype, per_face, closed, first, capacity):
        L, closed = capi.load(), int(bool(closed))
        return _fetch_all(lambda at, n, out, total: check(L.vrc_volume_extract_surface(self._h, closed, fmt, at, n, out, total, capi.VRC_MEM_HOST, None)),
                          first, capacity, per_face, dtype, self.SURFACE_WINDOW)

    def surfaceFaces(self, closed=True, first=0, capacity=None):
        """(n, 4) uint32 x y z d: the exposed faces [first, first + capacity) of the canonical order (by occupancy word,
        direction, bit), each named by its SOLID voxel and direction.  capacity=None fetches everything from `first` on in
        bounded windows.  Synchronous."""
        return self._surface(capi.VRC_SURFACE_FACES, np.uint32, 4, closed, first, capacity)

    def surfaceTriangles(self, closed=True, first=0, capacity=None):
        """(2n, 9) int32: two triangles per face of the same window in xorMesh's fixed point (64 units per voxel), wound
        counter-clockwise seen from outside.  With closed=True the mesh is closed: xorMesh of it into an empty volume of the
        same depth gives this volume's voxel set back."""
        return self._surface(capi.VRC_SURFACE_TRIANGLES, np.int32, 18, closed, first, capacity).reshape(-1, 9)

    def extractSurfaceDevice(self, format, first, capacity, out_ptr, total_ptr, closed=True, stream=None):
        """the same window into device memory (16 bytes per face, or 72 for its two triangles), asynchronous on `stream`;
        total_ptr (may be None): a device uint64 that receives the number of faces in stream order"""
        check(capi.load().vrc_volume_extract_surface(self._h, int(bool(closed)), int(format), int(first), int(capacity), ptr(out_ptr), ptr(total_ptr),
                                                     capi.VRC_MEM_DEVICE, ptr(stream)))

    # ---- the solid voxels as a coordinate list (include/vrc.h: vrc_voxels_extract) ----

    @staticmethod
    def _box(box):
        if box is None:
            return None
        b = np.ascontiguousarray(box, np.uint32).reshape(-1)
        if b.shape[0] != 6:
            raise ValueError("a box is 6 numbers: lo (inclusive), hi (exclusive)")
        return b

    def voxelCount(self, which=capi.VRC_VOXELS_ALL, box=None, closed=True):
        """How many voxels voxels() with the same arguments lists.  Synchronous."""
        n = C.c_uint64()
        check(capi.load().vrc_voxels_count(self._h, int(which), int(bool(closed)), ptr(self._box(box)), C.byref(n)))
        return n.value

    def voxels(self, which=capi.VRC_VOXELS_ALL, box=None, neighbours=False, closed=True, first=0, capacity=None):
        """(n, 3) uint32 x y z -- setVoxels' input form -- or with neighbours=True (n, 4) x y z m: the solid voxels (which =
        capi.VRC_VOXELS_ALL), those with an empty face neighbour (_SURFACE) or those without (_INTERIOR) inside `box` (lo
        inclusive, hi exclusive; None: the whole volume), [first, first + capacity) of the ascending key order.  m is the
        27-bit neighbourhood mask (neighbour_bit, face_exposure, corner_occlusion); closed=False lets everything beyond the
        volume read solid.  capacity=None fetches everything from `first` on in bounded windows.  Synchronous."""
        L, closed, which, box = capi.load(), int(bool(closed)), int(which), self._box(box)
        fmt, per = (capi.VRC_VOXELS_NEIGHBOURS, 4) if neighbours else (capi.VRC_VOXELS_XYZ, 3)
        return _fetch_all(lambda at, n, out, total: check(L.vrc_voxels_extract(self._h, which, closed, ptr(box), fmt, at, n, out, total, capi.VRC_MEM_HOST, None)),
                          first, capacity, per, np.uint32, self.SURFACE_WINDOW)

    def surfaceVoxels(self, box=None, neighbours=False, closed=True, first=0, capacity=None):
        """voxels() of the solid voxels with at least one exposed face"""
        return self.voxels(capi.VRC_VOXELS_SURFACE, box, neighbours, closed, first, capacity)

    def extractVoxelsDevice(self, which, format, first, capacity, out_ptr, total_ptr, box=None, closed=True, stream=None):
        """the same window into device memory (12 bytes per voxel for capi.VRC_VOXELS_XYZ, 16 for _NEIGHBOURS, which wants a
        16-byte aligned buffer), asynchronous on `stream`; total_ptr (may be None): a device uint64 that receives the number
        of voxels in stream order.  An XYZ list can go straight into setVoxelsDevice on the same stream."""
        check(capi.load().vrc_voxels_extract(self._h, int(which), int(bool(closed)), ptr(self._box(box)), int(format), int(first), int(capacity),
                                             ptr(out_ptr), ptr(total_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    # ---- the same surface with coplanar faces merged into rectangles (include/vrc.h: vrc_extract_rects) ----

    def rectCount(self, closed=True):
        """(6,) uint64: rectangles per direction d = 2 * axis + side: the exposed faces of surfaceCount merged by the
        identical-run rule of include/vrc.h.  Synchronous."""
        out = np.zeros(6, np.uint64)
        check(capi.load().vrc_rect_count(self._h, int(bool(closed)), ptr(out)))
        return out

    def _rects(self, fmt, dtype, per_rect, closed, first, capacity):
        L, closed = capi.load(), int(bool(closed))
        return _fetch_all(lambda at, n, out, total: check(L.vrc_extract_rects(self._h, closed, fmt, at, n, out, total, capi.VRC_MEM_HOST, None)),
                          first, capacity, per_rect, dtype, self.SURFACE_WINDOW)

    def surfaceRects(self, closed=True, first=0, capacity=None):
        """(n, 4) uint32 x y z w: the rectangles [first, first + capacity) of the order (d, c_a, s0, r0), each named by its
        voxel of smallest coordinates and w = d | (nr - 1) << 8 | (ns - 1) << 20 (unpackRects takes it apart).
        capacity=None fetches everything from `first` on in bounded windows.  Synchronous."""
        return self._rects(capi.VRC_SURFACE_FACES, np.uint32, 4, closed, first, capacity)

    @staticmethod
    def unpackRects(records):
        """(n, 4) packed rectangle records -> (n, 6) int64 x y z d nr ns: nr the extent along the run axis, ns along the
        stack axis (x faces: y stacks, z runs; y faces: x stacks, z runs; z faces: x stacks, y runs)"""
        r = np.asarray(records, np.int64).reshape(-1, 4)
        w = r[:, 3]
        return np.stack([r[:, 0], r[:, 1], r[:, 2], w & 0xff, ((w >> 8) & 0x3ff) + 1, ((w >> 20) & 0x3ff) + 1], axis=1)

    def rectTriangles(self, closed=True, first=0, capacity=None):
        """(2n, 9) int32: two triangles per rectangle of the same window in xorMesh's fixed point, wound counter-clockwise
        seen from outside.  With closed=True xorMesh of them into an empty volume of the same depth gives this volume's
        voxel set back, as surfaceTriangles' do."""
        return self._rects(capi.VRC_SURFACE_TRIANGLES, np.int32, 18, closed, first, capacity).reshape(-1, 9)

    def extractRectsDevice(self, format, first, capacity, out_ptr, total_ptr, closed=True, stream=None):
        """the same window into device memory (16 bytes per rectangle, or 72 for its two triangles), asynchronous on
        `stream`; total_ptr (may be None): a device uint64 that receives the number of rectangles in stream order"""
        check(capi.load().vrc_extract_rects(self._h, int(bool(closed)), int(format), int(first), int(capacity), ptr(out_ptr), ptr(total_ptr),
                                                   capi.VRC_MEM_DEVICE, ptr(stream)))

    @staticmethod
    def meshFromFaces(faces, merged=False):
        """(n, 4) x y z d face records -> (verts (m, 3) int32 in voxel units, quads (n, 4) int64 indices): every distinct
        corner once, each quad wound counter-clockwise seen from outside.  merged=True takes the packed rectangle records
        of surfaceRects instead and gives one quad per rectangle; rectangles share the corners they have in common.  Host
        arithmetic."""
        f = np.asarray(faces, np.int64).reshape(-1, 4)
        n = f.shape[0]
        d = f[:, 3] & 0xff if merged else f[:, 3]
        a, s = d >> 1, d & 1
        u, w = (a + 1) % 3, (a + 2) % 3
        rows = np.arange(n)
        extent = np.ones((n, 3), np.int64)
        if merged:
            r = np.where(a == 0, 2, np.where(a == 1, 2, 1))          # the run axis; the stack axis is the one left over
            extent[rows, r] = ((f[:, 3] >> 8) & 0x3ff) + 1
            extent[rows, 3 - a - r] = ((f[:, 3] >> 20) & 0x3ff) + 1
        du, dw = np.array([0, 1, 1, 0]), np.array([0, 0, 1, 1])
        corners = np.zeros((n, 4, 3), np.int64)
        for k in range(4):
            j = np.where(s == 1, k, (4 - k) % 4)         # q0 q1 q2 q3 towards +axis, q0 q3 q2 q1 towards -axis
            corners[rows, k, a] = f[rows, a] + s
            corners[rows, k, u] = f[rows, u] + du[j] * extent[rows, u]
            corners[rows, k, w] = f[rows, w] + dw[j] * extent[rows, w]
        verts, index = np.unique(corners.reshape(-1, 3), axis=0, return_inverse=True)
        return verts.astype(np.int32).reshape(-1, 3), np.asarray(index, np.int64).reshape(n, 4)

    def toMesh(self, closed=True, merged=False):
        """The exposed faces as an indexed quad mesh (verts, quads), see meshFromFaces; merged=True gives one quad per
        rectangle of surfaceRects.  scenes.write_obj writes it out."""
        return self.meshFromFaces(self.surfaceRects(closed) if merged else self.surfaceFaces(closed), merged)

    def commit(self, textures=None):
        """A NEW LSVO of the current occupancy (build_ms = device time of the sweeps); the volume stays editable."""
        handle, ms = C.c_void_p(), C.c_float()
        check(capi.load().vrc_volume_commit(self._h, C.byref(handle), C.byref(ms)))
        svo = LSVO._from_handle(handle, self.depth, self.device, textures)
        svo.build_ms = ms.value
        return svo

    def download(self):
        """dense uint8 [x, y, z] occupancy (0 / 1)"""
        size = 1 << self.depth
        out = np.zeros((size, size, size), np.uint8)
        check(capi.load().vrc_volume_download(self._h, ptr(out)))
        return out

    def solidCount(self):
        n = C.c_uint64()
        check(capi.load().vrc_volume_solid_count(self._h, C.byref(n)))
        return int(n.value)

    def packInfo(self):
        """What pack() would write, as a capi.PackInfo (bytes, mixed_tiles, full_tiles, partial_bricks, solid, ...): the
        count and scan passes alone (include/vrc.h: vrc_pack_volume with no buffer).  Synchronous."""
        info = capi.PackInfo()
        check(capi.load().vrc_pack_volume(self._h, None, 0, C.byref(info), capi.VRC_MEM_HOST))
        return info

    def pack(self, device=False):
        """The volume as its sparse tile stream (include/vrc.h: the format, version 1): a uint8 numpy array, or with
        device=True a uint8 torch tensor on the volume's device that the stream never leaves.  Equal occupancies give equal
        bytes.  Synchronous."""
        info = self.packInfo()
        n = int(info.bytes)
        if device:
            import torch
            out = torch.empty(n, dtype=torch.uint8, device="cuda:%d" % self.device)
            check(capi.load().vrc_pack_volume(self._h, ptr(out.data_ptr()), n, C.byref(info), capi.VRC_MEM_DEVICE))
            return out
        out = np.empty(n, np.uint8)
        check(capi.load().vrc_pack_volume(self._h, ptr(out), n, C.byref(info), capi.VRC_MEM_HOST))
        return out

    def unpack(self, data):
        """Replaces the whole occupancy by the one of a stream made by pack(): bytes, a uint8 numpy array, or a uint8 torch
        tensor on the volume's device (read in place).  A stream that breaks a canonical rule raises VrcError naming the rule
        and leaves the volume as it was.  Synchronous."""
        if hasattr(data, "data_ptr"):
            if not data.is_cuda:
                data = data.numpy()
            else:
                data = data.contiguous()
                check(capi.load().vrc_unpack_volume(self._h, ptr(data.data_ptr()), int(data.numel()), capi.VRC_MEM_DEVICE))
                return
        data = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, np.uint8).reshape(-1)
        check(capi.load().vrc_unpack_volume(self._h, ptr(data), data.size, capi.VRC_MEM_HOST))

    def save(self, path):
        """writes pack() to a file; returns its capi.PackInfo"""
        stream = self.pack()
        with open(path, "wb") as f:
            f.write(stream.tobytes())
        return packed_info(stream)

    @classmethod
    def fromPacked(cls, data, device=0):
        """A new volume from a stream (bytes, numpy array or device tensor as for unpack); the depth is the header's."""
        volume = cls(int(packed_info(data).depth), device)
        try:
            volume.unpack(data)
        except Exception:
            volume.close()
            raise
        return volume

    @classmethod
    def load(cls, path, device=0):
        """A new volume from a file written by save()."""
        with open(path, "rb") as f:
            return cls.fromPacked(f.read(), device)

    def editScratchBytes(self):
        """device bytes in the scratch blocks of the edit calls (staging, flood, mark field, surface offsets, rectangle block, pack slots); include/vrc.h"""
        n = C.c_uint64()
        check(capi.load().vrc_volume_edit_scratch_bytes(self._h, C.byref(n)))
        return int(n.value)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_volume_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VoxelLabels:
    """The component id of every voxel of M, resident on the device (include/vrc.h: vrc_labels_*): a snapshot made by
    VoxelVolume.labelComponents or VoxelVolume.fracture.  Ids run 0 .. count-1 by ascending key of each piece's first voxel."""

    def __init__(self, handle, count, depth, device):
        self._h, self.count, self.depth, self.device = handle, count, depth, device

    def components(self, first=0, capacity=None):
        """the records [first, first + capacity) that exist, as capi.COMPONENT_DTYPE (first, lo, hi, voxels)"""
        return _fetch_known(lambda at, n, out: check(capi.load().vrc_labels_components(self._h, at, n, out, capi.VRC_MEM_HOST, None)),
                            self.count, first, capacity, capi.COMPONENT_DTYPE)

    def componentsDevice(self, first, capacity, out_ptr, stream=None):
        check(capi.load().vrc_labels_components(self._h, first, capacity, ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def at(self, xyz):
        """uint32 id per (n, 3) voxel coordinate, capi.VRC_NO_COMPONENT outside M or outside the volume"""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        out = np.zeros(xyz.shape[0], np.uint32)
        check(capi.load().vrc_labels_at(self._h, xyz.shape[0], ptr(xyz), ptr(out), capi.VRC_MEM_HOST, None))
        return out

    def atDevice(self, n, xyz_ptr, ids_ptr, stream=None):
        check(capi.load().vrc_labels_at(self._h, n, ptr(xyz_ptr), ptr(ids_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def select(self, keep, dst=None, op=capi.VRC_COPY_REPLACE):
        """dst (a new volume with None) becomes / gains / loses the voxels of the pieces with keep[id] != 0; returns dst"""
        keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
        if len(keep) != self.count:
            raise ValueError(f"keep has {len(keep)} entries for {self.count} components")
        if dst is None:
            dst = VoxelVolume(self.depth, self.device)
        check(capi.load().vrc_labels_select(self._h, ptr(keep) if self.count else None, dst._h, int(op), capi.VRC_MEM_HOST, None))
        return dst

    def selectDevice(self, keep_ptr, dst, op=capi.VRC_COPY_REPLACE, stream=None):
        """the same with `count` bytes of keep in device memory, asynchronous on `stream`"""
        check(capi.load().vrc_labels_select(self._h, ptr(keep_ptr), dst._h, int(op), capi.VRC_MEM_DEVICE, ptr(stream)))

    def fall(self, fixed=None, direction=None, drop_limit=0):
        """How far every piece can fall as a rigid body along `direction` (a capi.VRC_FACE_* code; on the terrain generator's
        scenes down is capi.VRC_FACE_YN) before it meets a solid voxel of the volume `fixed` (None: nothing), the volume's
        face, drop_limit (0 = none) or a piece that has come to rest -- include/vrc.h: vrc_fall_drops.  Returns
        ((count, 3) int32 offsets, capi.FallStats).  Synchronous."""
        if direction is None:
            raise TypeError("fall: direction has no default -- which way is down is the caller's business (capi.VRC_FACE_*)")
        offsets, stats = np.zeros((self.count, 3), np.int32), capi.FallStats()
        check(capi.load().vrc_fall_drops(self._h, fixed._h if fixed is not None else None, int(direction), int(drop_limit),
                                          ptr(offsets) if self.count else None, capi.VRC_MEM_HOST, C.byref(stats)))
        return offsets, stats

    def fallDevice(self, offsets_ptr, fixed=None, direction=None, drop_limit=0):
        """the same with the count x 3 int32 offsets written to device memory, for placeDevice; still synchronous"""
        if direction is None:
            raise TypeError("fallDevice: direction has no default -- which way is down is the caller's business (capi.VRC_FACE_*)")
        stats = capi.FallStats()
        check(capi.load().vrc_fall_drops(self._h, fixed._h if fixed is not None else None, int(direction), int(drop_limit), ptr(offsets_ptr),
                                          capi.VRC_MEM_DEVICE, C.byref(stats)))
        return stats

    def place(self, offsets, dst=None, op=capi.VRC_COPY_OR, keep=None):
        """dst (a new volume with None) gains (VRC_COPY_OR) or loses (VRC_COPY_ANDNOT) every voxel of the pieces with
        keep[id] != 0 (None: all), each piece moved by its own (count, 3) int32 offset; what leaves the volume is dropped.
        Returns dst."""
        offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1, 3)
        if len(offsets) != self.count:
            raise ValueError(f"offsets has {len(offsets)} rows for {self.count} components")
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
            if len(keep) != self.count:
                raise ValueError(f"keep has {len(keep)} entries for {self.count} components")
        if dst is None:
            dst = VoxelVolume(self.depth, self.device)
        check(capi.load().vrc_fall_place(self._h, ptr(keep), ptr(offsets) if self.count else None, dst._h, int(op), capi.VRC_MEM_HOST, None))
        return dst

    def placeDevice(self, offsets_ptr, dst, op=capi.VRC_COPY_OR, keep_ptr=None, stream=None):
        """the same with the offsets (and `count` bytes of keep) in device memory, asynchronous on `stream`"""
        check(capi.load().vrc_fall_place(self._h, ptr(keep_ptr), ptr(offsets_ptr), dst._h, int(op), capi.VRC_MEM_DEVICE, ptr(stream)))
        return dst

    def moments(self, first=0, capacity=None):
        """the raw moments of the pieces [first, first + capacity) that exist, as capi.MOMENTS_DTYPE: voxels, s1 (the sums of
        c = 2p + 1 per axis) and s2 (the sums of c_x c_x, c_y c_y, c_z c_z, c_x c_y, c_x c_z, c_y c_z) -- include/vrc.h:
        vrc_rigid_moments.  Exact integers."""
        return _fetch_known(lambda at, n, out: check(capi.load().vrc_rigid_moments(self._h, at, n, out, capi.VRC_MEM_HOST, None)),
                            self.count, first, capacity, capi.MOMENTS_DTYPE)

    def momentsDevice(self, first, capacity, out_ptr, stream=None):
        """the same into device memory (80 bytes a record), asynchronous on `stream`"""
        check(capi.load().vrc_rigid_moments(self._h, first, capacity, ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def massProperties(self, first=0, capacity=None):
        """(mass, centre of mass, inertia tensor about it) of the pieces of the window, float64 arrays of shapes (k,), (k, 3)
        and (k, 3, 3): mass_properties of moments()."""
        return mass_properties(self.moments(first, capacity))

    def poses(self, rot, dst_pivot, src_pivot=None, scale=1.0, dst_depth=None):
        """(maps, boxes) for placeAffine: piece i turned by rot (9 floats for all, or (count, 9); make_rotation's layout) and
        resized by `scale` (one, or one per piece) about src_pivot[i] -- its centre of mass by default -- which lands on
        dst_pivot[i] ((count, 3), continuous voxel coordinates of a volume of dst_depth, the labels' depth by default).  maps is
        a capi.AFFINE_DTYPE array, boxes (count, 6) uint32: vrc_affine_place_box of every piece's record box."""
        rot = np.ascontiguousarray(rot, np.float32)
        rot = np.broadcast_to(rot.reshape(-1, 9), (self.count, 9))
        scale = np.broadcast_to(np.asarray(scale, np.float32).reshape(-1), (self.count,))
        dst_pivot = np.ascontiguousarray(dst_pivot, np.float32).reshape(self.count, 3)
        if src_pivot is None:
            src_pivot = self.massProperties()[1]
        src_pivot = np.ascontiguousarray(src_pivot, np.float32).reshape(self.count, 3)
        records = self.components()
        maps, boxes = np.zeros(self.count, capi.AFFINE_DTYPE), np.zeros((self.count, 6), np.uint32)
        for i in range(self.count):
            a, lo, hi = affine_place_box(rot[i], scale[i], src_pivot[i], dst_pivot[i], records["lo"][i], records["hi"][i],
                                         self.depth if dst_depth is None else dst_depth)
            maps[i] = (list(a.m), a.reserved, list(a.t))
            boxes[i] = lo + hi
        return maps, boxes

    def placeAffine(self, maps, boxes=None, dst=None, op=capi.VRC_COPY_OR, keep=None):
        """dst (a new volume of the labels' depth with None; any depth otherwise) gains (VRC_COPY_OR) or loses
        (VRC_COPY_ANDNOT) every piece with keep[id] != 0 (None: all), each read through its OWN inverse map inside its own box
        of dst ((count, 6) uint32 lo, hi; None: all of dst) -- include/vrc.h: vrc_rigid_place_affine.  maps: count capi.Affine
        or a capi.AFFINE_DTYPE array, e.g. from poses().  Returns dst."""
        maps = affine_array(maps)
        if len(maps) != self.count:
            raise ValueError(f"maps has {len(maps)} entries for {self.count} components")
        if boxes is not None:
            boxes = np.ascontiguousarray(boxes, np.uint32).reshape(-1, 6)
            if len(boxes) != self.count:
                raise ValueError(f"boxes has {len(boxes)} rows for {self.count} components")
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
            if len(keep) != self.count:
                raise ValueError(f"keep has {len(keep)} entries for {self.count} components")
        if dst is None:
            dst = VoxelVolume(self.depth, self.device)
        check(capi.load().vrc_rigid_place_affine(self._h, ptr(keep), ptr(maps) if self.count else None, ptr(boxes), dst._h, int(op), capi.VRC_MEM_HOST, None))
        return dst

    def placeAffineDevice(self, maps_ptr, dst, boxes_ptr=None, op=capi.VRC_COPY_OR, keep_ptr=None, stream=None):
        """the same with the maps (64 bytes each), the boxes and `count` bytes of keep in device memory, asynchronous on
        `stream`; a piece whose map lies beyond the limits is dropped whole"""
        check(capi.load().vrc_rigid_place_affine(self._h, ptr(keep_ptr), ptr(maps_ptr), ptr(boxes_ptr), dst._h, int(op), capi.VRC_MEM_DEVICE, ptr(stream)))
        return dst

    def _contact_arguments(self, maps, boxes, keep):
        maps = affine_array(maps)
        if len(maps) != self.count:
            raise ValueError(f"maps has {len(maps)} entries for {self.count} components")
        if boxes is not None:
            boxes = np.ascontiguousarray(boxes, np.uint32).reshape(-1, 6)
            if len(boxes) != self.count:
                raise ValueError(f"boxes has {len(boxes)} rows for {self.count} components")
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
            if len(keep) != self.count:
                raise ValueError(f"keep has {len(keep)} entries for {self.count} components")
        return maps, boxes, keep

    def contacts(self, maps, world, boxes=None, keep=None):
        """One capi.CONTACT_DTYPE record per piece: piece i read through its OWN inverse map inside its own box ((count, 6)
        uint32 lo, hi; None: all of world), as placeAffine would write it into a volume of world's depth, against the solid
        voxels of `world` and its faces -- include/vrc.h: vrc_rigid_contacts.  posed = its voxels there, overlap* = those inside
        the world's solid (count, sum of c = 2p + 1, sum of normals), touch* = those outside it with a solid voxel or a face of
        the volume next to them.  A piece with keep[id] == 0 (None: all kept) or an empty box has an all-zero record.  world is
        only read; nothing is excluded from it, so against the labelled medium itself a piece at rest overlaps itself."""
        maps, boxes, keep = self._contact_arguments(maps, boxes, keep)
        out = np.zeros(self.count, capi.CONTACT_DTYPE)
        check(capi.load().vrc_rigid_contacts(self._h, ptr(keep), ptr(maps) if self.count else None, ptr(boxes), world._h,
                                              ptr(out) if self.count else None, capi.VRC_MEM_HOST, None))
        return out

    def contactsDevice(self, maps_ptr, world, out_ptr, boxes_ptr=None, keep_ptr=None, stream=None):
        """the same with the maps (64 bytes each), the boxes, `count` bytes of keep and the records (128 bytes each) in device
        memory, asynchronous on `stream`; a piece whose map lies beyond the limits has an all-zero record"""
        check(capi.load().vrc_rigid_contacts(self._h, ptr(keep_ptr), ptr(maps_ptr), ptr(boxes_ptr), world._h, ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def candidatePairs(self, boxes, depth=None, keep=None):
        """The broad phase of pairContacts (include/vrc.h: vrc_rigid_box_pairs): the ordered pairs (a, b), a != b, of pieces with
        keep[id] != 0 (None: all) whose (count, 6) uint32 boxes, clipped to a posed volume of `depth` (None: the labels'), meet
        when one is grown by a voxel -- necessary for overlap or touch.  Both orders, ascending; a (P, 2) uint32 array."""
        depth = self.depth if depth is None else int(depth)
        boxes = np.ascontiguousarray(boxes, np.uint32).reshape(-1, 6)
        if len(boxes) != self.count:
            raise ValueError(f"boxes has {len(boxes)} rows for {self.count} components")
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
            if len(keep) != self.count:
                raise ValueError(f"keep has {len(keep)} entries for {self.count} components")
        count = C.c_uint64()
        check(capi.load().vrc_rigid_box_pair_count(self._h, ptr(keep), ptr(boxes) if self.count else None, depth, C.byref(count), capi.VRC_MEM_HOST, None))
        pairs = np.zeros((int(count.value), 2), np.uint32)
        if len(pairs):
            check(capi.load().vrc_rigid_box_pairs(self._h, ptr(keep), ptr(boxes), depth, 0, len(pairs), ptr(pairs), capi.VRC_MEM_HOST, None))
        return pairs

    def pairContacts(self, maps, pairs=None, boxes=None, depth=None, keep=None):
        """One capi.CONTACT_DTYPE record per ordered pair (a, b) of the (P, 2) uint32 `pairs`: piece a, posed as placeAffine
        would write it into a volume of `depth` (None: the labels'), against piece b posed the same way and nothing else -- no
        world and no walls -- include/vrc.h: vrc_rigid_pair_contacts.  posed = a's voxels there, overlap* = those inside b,
        touch* = those outside b with a voxel of b next to them; the normals point out of b.  List (b, a) as well for b's side.
        pairs=None: candidatePairs(boxes, depth, keep) first, which needs boxes; call that yourself to keep the list."""
        maps, boxes, keep = self._contact_arguments(maps, boxes, keep)
        depth = self.depth if depth is None else int(depth)
        if pairs is None:
            if boxes is None:
                raise ValueError("pairContacts: pairs=None needs boxes for candidatePairs")
            pairs = self.candidatePairs(boxes, depth, keep)
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        out = np.zeros(len(pairs), capi.CONTACT_DTYPE)
        check(capi.load().vrc_rigid_pair_contacts(self._h, ptr(keep), ptr(maps) if self.count else None, ptr(boxes), depth, len(pairs),
                                                   ptr(pairs) if len(pairs) else None, ptr(out) if len(pairs) else None, capi.VRC_MEM_HOST, None))
        return out

    def pairContactsDevice(self, maps_ptr, n_pairs, pairs_ptr, out_ptr, boxes_ptr=None, depth=None, keep_ptr=None, stream=None):
        """the same with the maps, the boxes, `count` bytes of keep, the n_pairs x 2 uint32 pairs and the records (128 bytes each)
        in device memory, asynchronous on `stream`; a pair with a piece index beyond the pieces, or whose first piece has a map
        beyond the limits, has an all-zero record"""
        check(capi.load().vrc_rigid_pair_contacts(self._h, ptr(keep_ptr), ptr(maps_ptr), ptr(boxes_ptr), self.depth if depth is None else int(depth),
                                                   int(n_pairs), ptr(pairs_ptr), ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def collides(self, maps, world, boxes=None, keep=None):
        """bool per piece: the posed piece shares a voxel with the world's solid (contacts()["overlap"] > 0)"""
        return self.contacts(maps, world, boxes, keep)["overlap"] > 0

    def clearance(self, maps, field, boxes=None, keep=None):
        """One capi.CLEARANCE_DTYPE record per piece: `field` (a VoxelDistance, Euclidean or travel, of any depth) read at the
        voxels of piece i posed as contacts() poses it into a volume of the field's depth -- include/vrc.h:
        vrc_rigid_clearance.  posed = its voxels there, none = those whose value is capi.VRC_DISTANCE_NONE, sum = the sum of the
        finite values, min_value / max_value = the least / greatest finite one (VRC_DISTANCE_NONE / 0 without any) and min_at /
        max_at the voxel of smallest dense index that holds it.  A piece with keep[id] == 0 (None: all kept) or an empty box
        has the record of the empty set: min_value VRC_DISTANCE_NONE, the rest 0."""
        maps, boxes, keep = self._contact_arguments(maps, boxes, keep)
        out = np.zeros(self.count, capi.CLEARANCE_DTYPE)
        check(capi.load().vrc_rigid_clearance(self._h, ptr(keep), ptr(maps) if self.count else None, ptr(boxes), field._h,
                                               ptr(out) if self.count else None, capi.VRC_MEM_HOST, None))
        return out

    def clearanceDevice(self, maps_ptr, field, out_ptr, boxes_ptr=None, keep_ptr=None, stream=None):
        """the same with the maps (64 bytes each), the boxes, `count` bytes of keep and the records (64 bytes each) in device
        memory, asynchronous on `stream`; a piece whose map lies beyond the limits has the record of the empty set"""
        check(capi.load().vrc_rigid_clearance(self._h, ptr(keep_ptr), ptr(maps_ptr), ptr(boxes_ptr), field._h, ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def freeRadius(self, maps, field, boxes=None, keep=None):
        """int64 per piece, from clearance()["min_value"] over the squared distance to a feature set: the largest r such that
        every integer translation o of the posed piece with |o| <= r stays clear of the set -- isqrt(min_value - 1); -1 where
        min_value is 0 (the piece already overlaps the set); the field's S where there is no finite value (nothing to hit)"""
        return free_radius(self.clearance(maps, field, boxes, keep)["min_value"], 1 << field.depth)

    def pieceSites(self, first=0, capacity=None):
        """uint32 per piece of [first, first + capacity) that exists: the index of the site whose cell the piece lies in,
        capi.VRC_NO_COMPONENT for "none" -- labels made by VoxelVolume.fracture only (include/vrc.h: vrc_fracture_piece_sites)"""
        return _fetch_known(lambda at, n, out: check(capi.load().vrc_fracture_piece_sites(self._h, at, n, out, capi.VRC_MEM_HOST, None)),
                            self.count, first, capacity, np.uint32)

    def pieceSitesDevice(self, first, capacity, out_ptr, stream=None):
        """the same into device memory, asynchronous on `stream`"""
        check(capi.load().vrc_fracture_piece_sites(self._h, first, capacity, ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def bytes(self):
        return int(capi.load().vrc_labels_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_labels_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VoxelDistance:
    """The squared Euclidean distance of every voxel to the feature set, resident on the device as S^3 uint32 in
    [(x*S + y)*S + z] order (include/vrc.h: vrc_distance_*): a snapshot made by VoxelVolume.distanceField.  `stats` is a
    capi.DistanceStats (features, max_d2, argmax).  VoxelVolume.travelField makes the same object with the steps from the
    seeds in place of the squared distance: `stats` is then a capi.TravelStats and `connectivity` 6 or 26, not 0."""

    def __init__(self, handle, stats, depth, device):
        self._h, self.stats, self.depth, self.device = handle, stats, depth, device

    @property
    def connectivity(self):
        """6 or 26 for a travel field, 0 for a Euclidean one"""
        return int(capi.load().vrc_travel_connectivity(self._h))

    def tracePaths(self, starts, capacity=None):
        """Routes off a travel field (include/vrc.h: vrc_travel_trace_paths): (lengths, routes) for (n, 3) start voxels --
        lengths[i] = the field at start i, capi.VRC_DISTANCE_NONE outside the volume or where nothing arrives; routes[i] a
        (k, 3) uint32 array from the start towards a seed, k = min(length, capacity - 1) + 1 voxels, empty for a start without
        a value.  capacity=None sizes the rows by the longest route, so every route ends at a seed."""
        starts = np.ascontiguousarray(starts, np.uint32).reshape(-1, 3)
        n = starts.shape[0]
        lengths = np.zeros(n, np.uint32)
        if capacity is None:
            if n:
                check(capi.load().vrc_travel_trace_paths(self._h, n, ptr(starts), 0, None, ptr(lengths), capi.VRC_MEM_HOST, None))
            finite = lengths[lengths != capi.VRC_DISTANCE_NONE]
            capacity = int(finite.max()) + 1 if len(finite) else 0
        capacity = int(capacity)
        paths = np.zeros((n, capacity, 3), np.uint32)
        if n:
            check(capi.load().vrc_travel_trace_paths(self._h, n, ptr(starts), capacity, ptr(paths) if capacity else None, ptr(lengths),
                                                       capi.VRC_MEM_HOST, None))
        routes = []
        for i in range(n):
            k = 0 if lengths[i] == capi.VRC_DISTANCE_NONE or capacity == 0 else min(int(lengths[i]), capacity - 1) + 1
            routes.append(paths[i, :k].copy())
        return lengths, routes

    def tracePathsDevice(self, n, starts_ptr, capacity, paths_ptr, lengths_ptr, stream=None):
        """the same over n x 3 uint32 starts, n x capacity x 3 uint32 of routes and n uint32 lengths in device memory,
        asynchronous on `stream`; nothing beyond the voxels of a route is written"""
        check(capi.load().vrc_travel_trace_paths(self._h, n, ptr(starts_ptr), int(capacity), ptr(paths_ptr), ptr(lengths_ptr), capi.VRC_MEM_DEVICE,
                                                   ptr(stream)))

    @staticmethod
    def _sight_flags(touch, plain=False):
        return (capi.VRC_SIGHT_TOUCH if touch else 0) | (capi.VRC_SIGHT_PLAIN if plain else 0)

    def sight(self, a, b, lo=1, hi=capi.VRC_DISTANCE_NONE, touch=False, plain=False):
        """Straight walks over the field (include/vrc.h: vrc_sight_segments): one capi.SIGHT_DTYPE record per segment from
        voxel a[i] to voxel b[i] ((n, 3) each, or one voxel for all) -- status capi.VRC_SIGHT_CLEAR when every visited voxel has
        lo <= value <= hi, VRC_SIGHT_BLOCKED with `at` the first that has not and `before` the voxel visited before it,
        VRC_SIGHT_OUTSIDE for an endpoint outside the volume.  touch: the supercover, every voxel the segment touches, where
        the default passes diagonally between two voxels.  lo = r^2 + 1 on the field to the solid asks for a ball of radius
        r.  plain: never stride (the records are the same either way)."""
        a, b = np.asarray(a, np.int64).reshape(-1, 3), np.asarray(b, np.int64).reshape(-1, 3)
        n = max(len(a), len(b))
        segments = np.empty((n, 6), np.int32)
        segments[:, :3], segments[:, 3:] = a, b
        out = np.zeros(n, capi.SIGHT_DTYPE)
        check(capi.load().vrc_sight_segments(self._h, n, ptr(segments), int(lo), int(hi), self._sight_flags(touch, plain), ptr(out), capi.VRC_MEM_HOST, None))
        return out

    def sightDevice(self, n, segments_ptr, out_ptr, lo=1, hi=capi.VRC_DISTANCE_NONE, touch=False, plain=False, stream=None):
        """the same over n x 6 int32 of segments and n 32-byte records in device memory, asynchronous on `stream`"""
        check(capi.load().vrc_sight_segments(self._h, n, ptr(segments_ptr), int(lo), int(hi), self._sight_flags(touch, plain), ptr(out_ptr), capi.VRC_MEM_DEVICE,
                                             ptr(stream)))

    def visibleFrom(self, eye, radius=0, lo=1, hi=capi.VRC_DISTANCE_NONE, touch=False, plain=False):
        """What an eye at voxel `eye` sees (include/vrc.h: vrc_sight_field): a new VoxelDistance holding |p - eye|^2 at every
        voxel p within `radius` (0: no limit) whose walk from the eye is clear up to, not counting, p itself, and
        capi.VRC_DISTANCE_NONE elsewhere; `stats` is a capi.SightStats (visible, max_d2, argmax).  One walk per voxel in
        range.  Synchronous."""
        eye = np.ascontiguousarray(eye, np.uint32).reshape(3)
        handle, stats = C.c_void_p(), capi.SightStats()
        check(capi.load().vrc_sight_field(self._h, ptr(eye), int(radius), int(lo), int(hi), self._sight_flags(touch, plain), C.byref(handle), C.byref(stats)))
        return VoxelDistance(handle, stats, self.depth, self.device)

    def bytes(self):
        return int(capi.load().vrc_distance_bytes(self._h))

    def data_ptr(self):
        """the device address of the field: an (S, S, S) uint32 tensor for whoever wraps it"""
        return int(capi.load().vrc_distance_data(self._h) or 0)

    def at(self, xyz):
        """uint32 squared distance per (n, 3) voxel coordinate, capi.VRC_DISTANCE_NONE outside the volume"""
        xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
        out = np.zeros(xyz.shape[0], np.uint32)
        check(capi.load().vrc_distance_at(self._h, xyz.shape[0], ptr(xyz), ptr(out), capi.VRC_MEM_HOST, None))
        return out

    def atDevice(self, n, xyz_ptr, d2_ptr, stream=None):
        check(capi.load().vrc_distance_at(self._h, n, ptr(xyz_ptr), ptr(d2_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def download(self):
        """the whole field as an (S, S, S) uint32 array"""
        S = 1 << self.depth
        out = np.empty((S, S, S), np.uint32)
        check(capi.load().vrc_distance_download(self._h, ptr(out)))
        return out

    def select(self, lo, hi, dst=None, op=capi.VRC_COPY_REPLACE, stream=None):
        """dst (a new volume with None) becomes / gains / loses the voxels with lo <= D <= hi; asynchronous on `stream`,
        ordered as an edit of dst.  Returns dst."""
        if dst is None:
            dst = VoxelVolume(self.depth, self.device)
        check(capi.load().vrc_distance_select(self._h, int(lo), int(hi), dst._h, int(op), ptr(stream)))
        return dst

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_distance_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def smoothPath(route, field, radius=0, touch=True):
    """Greedy string pulling of a route ((k, 3) voxels, as VoxelVolume.shortestPath or VoxelDistance.tracePaths return it)
    over `field`, the VoxelDistance to the solid: from the anchor -- first the route's start -- one batched sight() covers
    every later voxel of the route, the one of greatest index that a ball of `radius` reaches in a straight line becomes the
    next waypoint and anchor, until the end is reached.  Returns the waypoints, a subsequence of the route that keeps both
    ends.  Every leg that spans more than one step of the route is a clear segment.  Where no later voxel is reached in a
    clear line -- the next step of the route is not clear itself: the route runs closer to a wall than `radius`, or, with
    touch, takes a diagonal step past a corner -- that single step is kept as the leg, clear or not; check such legs with
    sight() if the route was not made for this radius."""
    route = np.ascontiguousarray(route, np.uint32).reshape(-1, 3)
    r = int(radius)
    if r < 0:
        raise ValueError(f"smoothPath: negative radius {r}")
    lo = min(r, 65535) ** 2 + 1
    keep, anchor = [0], 0
    while anchor < len(route) - 1:
        records = field.sight(route[anchor], route[anchor + 1:], lo=lo, touch=touch)
        clear = np.flatnonzero(records["status"] == capi.VRC_SIGHT_CLEAR)
        anchor += int(clear[-1]) + 1 if len(clear) else 1
        keep.append(anchor)
    return route[keep]


class VoxelDelta:
    """The difference of two volumes, resident on the device as records {word, bits} in ascending word order
    (include/vrc.h: vrc_delta_*): a snapshot made by VoxelVolume.diff or from caller records.  `stats` is a capi.DeltaStats
    (words, voxels, lo, hi -- the box of the changed voxels, hi exclusive), `count` the number of records.  Applying it
    (VoxelVolume.applyDelta) flips the changed voxels: it is its own inverse."""

    def __init__(self, handle, stats, depth, device):
        self._h, self.stats, self.depth, self.device = handle, stats, depth, device
        self.count = int(stats.words)

    @classmethod
    def fromRecords(cls, depth, records, device=0):
        """from capi.DELTA_RECORD_DTYPE records (or anything that reshapes to (n, 2) uint32: word, bits) in host memory --
        another rank's, a saved history's; a list that is not strictly ascending in word, names a word beyond the volume or
        holds bits == 0 raises VrcError with the first offending index"""
        records = np.asarray(records)
        if records.dtype != capi.DELTA_RECORD_DTYPE:
            records = np.ascontiguousarray(records, np.uint32).reshape(-1, 2)
        records = np.ascontiguousarray(records)
        return cls._create(depth, records.shape[0], ptr(records) if records.shape[0] else None, capi.VRC_MEM_HOST, device)

    @classmethod
    def fromRecordsDevice(cls, depth, n, records_ptr, device=0):
        """the same over n x 2 uint32 in device memory, copied into the object device to device; synchronous"""
        return cls._create(depth, n, ptr(records_ptr), capi.VRC_MEM_DEVICE, device)

    @classmethod
    def _create(cls, depth, n, records, mem, device):
        handle, stats = C.c_void_p(), capi.DeltaStats()
        check(capi.load().vrc_delta_create(int(depth), int(device), int(n), records, mem, C.byref(handle), C.byref(stats)))
        return cls(handle, stats, depth, device)

    def records(self, first=0, capacity=None):
        """the records [first, first + capacity) that exist, as capi.DELTA_RECORD_DTYPE (word, bits)"""
        return _fetch_known(lambda at, n, out: check(capi.load().vrc_delta_records(self._h, at, n, out, capi.VRC_MEM_HOST, None)),
                            self.count, first, capacity, capi.DELTA_RECORD_DTYPE)

    def recordsDevice(self, first, capacity, out_ptr, stream=None):
        """the same into device memory, asynchronous on `stream`"""
        check(capi.load().vrc_delta_records(self._h, first, capacity, ptr(out_ptr), capi.VRC_MEM_DEVICE, ptr(stream)))

    def bytes(self):
        return int(capi.load().vrc_delta_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_delta_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VoxelHistory:
    """Undo and redo for a VoxelVolume at the cost of what each step changed: one shadow clone of the volume and two stacks of
    VoxelDelta.  Edit the volume with any call, then record(); only record() reads the two occupancies, undo() and redo()
    cost what their delta holds.  max_bytes (None: no limit) bounds the record bytes of both stacks: record() drops the
    oldest undo steps beyond it, never the one it has just taken.  The deltas returned stay owned by the history."""

    def __init__(self, volume, max_bytes=None):
        self.volume, self.max_bytes = volume, max_bytes
        self._shadow = volume.clone()
        self._undo, self._redo = [], []

    def record(self):
        """the step from the state at the last record / undo / redo to the volume as it is now: its VoxelDelta, pushed on
        the undo stack (the redo stack is cleared), or None when nothing changed"""
        delta = self._shadow.diff(self.volume)
        if not delta.count:
            delta.close()
            return None
        self._shadow.applyDelta(delta)
        self._undo.append(delta)
        self._drop(self._redo, 0)
        if self.max_bytes is not None:
            while len(self._undo) > 1 and self.bytes() > self.max_bytes:
                self._drop(self._undo, len(self._undo) - 1)
        return delta

    def undo(self):
        """takes the last recorded step back; returns its VoxelDelta (stats.lo / hi: what to redraw), None with nothing to undo"""
        return self._move(self._undo, self._redo)

    def redo(self):
        """the mirror of undo()"""
        return self._move(self._redo, self._undo)

    def _move(self, source, sink):
        if not source:
            return None
        delta = source.pop()
        self.volume.applyDelta(delta)
        self._shadow.applyDelta(delta)
        sink.append(delta)
        return delta

    @staticmethod
    def _drop(stack, keep):
        """closes all but the newest `keep` entries"""
        while len(stack) > keep:
            stack.pop(0).close()

    @property
    def undoCount(self):
        return len(self._undo)

    @property
    def redoCount(self):
        return len(self._redo)

    def bytes(self):
        """record bytes held by both stacks (the shadow clone's occupancy is not counted)"""
        return sum(d.bytes() for d in self._undo + self._redo)

    def close(self):
        self._drop(self._undo, 0)
        self._drop(self._redo, 0)
        if self._shadow is not None:
            self._shadow.close()
            self._shadow = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Grid3D:
    """Dense grid (grid_3d.hpp); cells[x, y, z] = Cell::Type (0 = Empty)."""

    def __init__(self, cells, device=0):
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        X, Y, Z = cells.shape
        self._h = C.c_void_p()
        check(capi.load().vrc_grid_create(ptr(cells), X, Y, Z, device, C.byref(self._h)))

    def castRays(self, org, dir_):
        org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
        dir_ = np.ascontiguousarray(dir_, np.float32).reshape(-1, 3)
        out = np.zeros(org.shape[0], HIT_DTYPE)
        check(capi.load().vrc_grid_cast_rays(self._h, org.shape[0], ptr(org), ptr(dir_), ptr(out),
                                             capi.VRC_MEM_HOST, None))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_grid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fetch_all(call, first, capacity, per, dtype, window):
    """(n, per) records [first, first + capacity) of a windowed list whose total only the library knows (capacity=None:
    everything from `first` on).  call(first, n, out_ptr, total_ref) wraps the C entry point: one call with capacity 0 asks
    the total, then the records come in windows of at most `window`."""
    total = C.c_uint64()
    call(0, 0, None, C.byref(total))
    first = int(first)
    n = max(0, total.value - first)
    if capacity is not None:
        n = min(n, int(capacity))
    out = np.zeros((n, per), dtype)
    for at in range(0, n, window):
        part = out[at:at + window]
        call(first + at, part.shape[0], ptr(part), None)
    return out


def _fetch_known(call, count, first, capacity, dtype):
    """the records [first, first + capacity) that exist of a list of `count` records, in one call(first, n, out_ptr); an
    empty window still makes the call, with no buffer"""
    if capacity is None:
        capacity = max(count - first, 0)
    out = np.zeros(min(capacity, max(count - first, 0)), dtype)
    call(first, len(out), ptr(out) if len(out) else None)
    return out


def make_camera(position, rot, fov=1.0, aperture=0.0, focal_length=1.0):
    cam = Camera()
    cam.position[:] = [float(v) for v in position]
    cam.rot[:] = [float(v) for v in rot]
    cam.fov, cam.aperture, cam.focal_length = fov, aperture, focal_length
    return cam


class RayCaster:
    """raycaster.hpp:43-283 with the framebuffer and sample accumulators on the GPU."""

    def __init__(self, svo, render_size):
        self.svo = svo
        self.width, self.height = int(render_size[0]), int(render_size[1])
        self._h = C.c_void_p()
        check(capi.load().vrc_renderer_create(svo._h, self.width, self.height, C.byref(self._h)))
        self.light_position = (0.0, 0.0, 0.0)
        self.use_gi = False
        self.use_samples = False
        self.shadow_samples = 0      # 0 = reference default
        self.gi_bounces = 1
        self.seed = 0x9E3779B9
        self.frame_index = 0

    def setLightPosition(self, position):
        self.light_position = tuple(float(v) for v in position)

    def setScene(self, svo):
        """The following frames walk `svo` (same depth, same device); image, accumulators and counters are kept."""
        check(capi.load().vrc_renderer_set_scene(self._h, svo._h))
        self.svo = svo

    def params(self, spp=1, checker_parity=-1, row_block=0, shard_index=0, shard_count=1):
        p = FrameParams()
        p.light_position[:] = self.light_position
        p.use_gi, p.use_samples = int(self.use_gi), int(self.use_samples)
        p.shadow_samples, p.gi_bounces = self.shadow_samples, self.gi_bounces
        p.checker_parity, p.spp = checker_parity, spp
        p.seed, p.frame_index = self.seed, self.frame_index
        p.row_block, p.shard_index, p.shard_count = row_block, shard_index, shard_count
        return p

    def renderFrame(self, camera, spp=1, checker_parity=-1, stream=None, row_block=0, shard_index=0, shard_count=1):
        p = self.params(spp, checker_parity, row_block, shard_index, shard_count)
        check(capi.load().vrc_render_frame(self._h, C.byref(camera), C.byref(p), ptr(stream)))
        self.frame_index += spp

    # scheduling knobs of THIS renderer (results never depend on them; see include/vrc.h)
    def setTuning(self, blocks_per_cu=0):
        check(capi.load().vrc_renderer_set_tuning(self._h, blocks_per_cu))

    def setSampleChunk(self, samples_per_unit):
        check(capi.load().vrc_renderer_set_sample_chunk(self._h, samples_per_unit))

    def lastKernel(self):
        """symbol of the frame kernel the last renderFrame* launched (what a rocprofv3 trace of the run lists)"""
        return capi.load().vrc_renderer_last_kernel(self._h).decode()

    def setWalkFromRoot(self, on=True):
        """Measurement switch: every ray from the root (none starts below it).  include/vrc.h: vrc_renderer_set_walk_from_root."""
        check(capi.load().vrc_renderer_set_walk_from_root(self._h, 1 if on else 0))

    def setLaneSamples(self, samples=0):
        """lane <-> (pixel, sample) map of the frame kernel: 1 = 8 x 8 pixels per wave, 4 = 4 x 4 pixels x 4 samples abreast,
        0 = the library's choice.  Same results either way.  include/vrc.h: vrc_renderer_set_lane_samples."""
        check(capi.load().vrc_renderer_set_lane_samples(self._h, samples))

    def setQuadWalks(self, on=True):
        """pinhole camera: the sample-invariant primary / shadow walks one quadrant of the tile at a time, four samples abreast (on
        by default where a launch allows it).  Same results.  include/vrc.h: vrc_renderer_set_quad_walks."""
        check(capi.load().vrc_renderer_set_quad_walks(self._h, 1 if on else 0))

    def setInvariantRayReuse(self, on=True):
        """beyond the reference: pinhole camera, walk a work unit's primary and shadow ray once instead of once per sample
        (same image; stats then count the walks executed).  include/vrc.h: vrc_renderer_set_invariant_ray_reuse."""
        check(capi.load().vrc_renderer_set_invariant_ray_reuse(self._h, 1 if on else 0))

    def renderFrameResolved(self, camera, spp=1, dst_ptr=None, stream=None, row_block=0, shard_index=0, shard_count=1):
        """renderFrame + resolveShard(..., reset=True) in one launch (vrc_render_frame_resolved): the frame's samples
        rendered, resolved into the image (and the packed shard buffer dst_ptr), accumulators left at zero."""
        p = self.params(spp, -1, row_block, shard_index, shard_count)
        check(capi.load().vrc_render_frame_resolved(self._h, C.byref(camera), C.byref(p), ptr(dst_ptr), ptr(stream)))
        self.frame_index += spp

    # ---- direct peer writes (include/vrc.h: vrc_ipc_*, vrc_renderer_set_image_target) ----
    def exportImage(self):
        """64 opaque bytes naming this renderer's framebuffer for the other processes of the node"""
        h = (C.c_ubyte * 64)()
        check(capi.load().vrc_ipc_export_image(self._h, C.byref(h)))
        return bytes(h)

    def setImageTarget(self, image_dev_ptr):
        """sharded sample-mode frames are resolved into that framebuffer (full-frame layout) instead of this renderer's own;
        None = own image again"""
        check(capi.load().vrc_renderer_set_image_target(self._h, ptr(image_dev_ptr)))

    def setPrimaryCapture(self, dev_ptr):
        check(capi.load().vrc_renderer_set_primary_capture(self._h, ptr(dev_ptr)))

    def samples_to_image(self, stream=None):
        check(capi.load().vrc_samples_to_image(self._h, ptr(stream)))

    def resetSamples(self, stream=None):
        check(capi.load().vrc_reset_samples(self._h, ptr(stream)))

    def clearImage(self, stream=None):
        check(capi.load().vrc_clear_image(self._h, ptr(stream)))

    def image_ptr(self):
        return capi.load().vrc_image_device_ptr(self._h)

    def readImage(self, stream=None):
        img = np.zeros((self.height, self.width, 4), np.uint8)
        check(capi.load().vrc_read_image(self._h, ptr(img), ptr(stream)))
        return img

    def writeImage(self, img, stream=None):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.shape == (self.height, self.width, 4)
        check(capi.load().vrc_write_image(self._h, ptr(img), ptr(stream)))

    def readAccum(self, stream=None):
        acc = np.zeros((self.height, self.width, 4), np.uint32)
        check(capi.load().vrc_read_accum(self._h, ptr(acc), ptr(stream)))
        return acc

    def stats(self, reset=False, stream=None):
        st = FrameStats()
        check(capi.load().vrc_get_stats(self._h, C.byref(st), int(reset), ptr(stream)))
        return st

    def packShard(self, row_block, shard_index, shard_count, dst_ptr, stream=None):
        check(capi.load().vrc_pack_shard(self._h, row_block, shard_index, shard_count, ptr(dst_ptr), ptr(stream)))

    def resolveShard(self, row_block=0, shard_index=0, shard_count=1, dst_ptr=None, reset=False, stream=None):
        """samples_to_image (+ packShard, + resetSamples) for this shard's rows in one kernel."""
        check(capi.load().vrc_resolve_shard(self._h, row_block, shard_index, shard_count, ptr(dst_ptr), int(reset), ptr(stream)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Presenter:
    """main.cpp:160-182 on the device: render_tex / denoised_tex persistence blend, nearest upscale to the window size,
    optional median (res/median_3.frag, res/median.frag).  Owns denoised_tex and the window image."""

    def __init__(self, render_size, window_size, device=0):
        self.width, self.height = int(render_size[0]), int(render_size[1])
        self.out_width, self.out_height = int(window_size[0]), int(window_size[1])
        self._h = C.c_void_p()
        check(capi.load().vrc_presenter_create(device, self.width, self.height, self.out_width, self.out_height, C.byref(self._h)))

    def present(self, raycaster, old_value_conservation=None, median=0, stream=None):
        """old_value_conservation defaults to main.cpp:161: use_samples ? 0 : 0.1"""
        if old_value_conservation is None:
            old_value_conservation = 0.0 if raycaster.use_samples else 0.1
        check(capi.load().vrc_present(self._h, raycaster._h, old_value_conservation, median, ptr(stream)))

    def presentImage(self, image_dev_ptr, old_value_conservation, median=0, stream=None):
        check(capi.load().vrc_present_image(self._h, ptr(image_dev_ptr), old_value_conservation, median, ptr(stream)))

    def clear(self, stream=None):
        check(capi.load().vrc_presenter_clear(self._h, ptr(stream)))

    def window_ptr(self):
        return capi.load().vrc_presenter_window_ptr(self._h)

    def read(self, stream=None):
        """(window RGBA8 (out_h, out_w, 4), denoised_tex RGBA8 (h, w, 4))"""
        win = np.zeros((self.out_height, self.out_width, 4), np.uint8)
        den = np.zeros((self.height, self.width, 4), np.uint8)
        check(capi.load().vrc_presenter_read(self._h, ptr(win), ptr(den), ptr(stream)))
        return win, den

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.load().vrc_presenter_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
