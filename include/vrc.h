/*
 * vrc.h -- C ABI of the MI355X-native voxel ray-traversal hot path
 * (drop-in for the per-ray / per-frame operators of johnBuffer/CpuVoxelRaycaster).
 *
 * Plain pointers and sizes only.  All citations are file:line under the
 * reference tree.  The library is libvrc_hip.so (cpuvoxelraycaster_amd/csrc);
 * every compute entry point runs hand-written HIP kernels for gfx950 and fails
 * with VRC_ERR_NO_DEVICE when no GPU is present -- there is no CPU fallback.
 *
 * Error convention (the reference has none to inherit: volumetric.hpp:55-61
 * has no error channel): every function returns 0 on success or a negative
 * VRC_ERR_* code; vrc_last_error() returns a thread-local message.
 *
 * Threading: a vrc_scene is immutable after creation and may be shared by
 * any number of renderers / threads (the reference calls castRay concurrently
 * from 16 workers, main.cpp:139-152).  A vrc_renderer is not re-entrant.  A
 * vrc_volume (the editable occupancy scenes are committed from) is not
 * re-entrant either: one thread at a time edits or commits it; the scenes it
 * has committed are ordinary immutable scenes.
 *
 * Streams: `stream` arguments are hipStream_t handles passed as void*
 * (NULL = the default stream).  Calls taking a stream are asynchronous on it
 * unless stated otherwise.
 */
#ifndef VRC_H
#define VRC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRC_OK                0
#define VRC_ERR_INVALID      -1   /* bad argument */
#define VRC_ERR_NO_DEVICE    -2   /* no HIP device / HIP runtime error at init */
#define VRC_ERR_HIP          -3   /* HIP runtime call failed (see vrc_last_error) */
#define VRC_ERR_OOM          -4
#define VRC_ERR_PEER         -5   /* a peer process of a direct-peer-write exchange died or timed out (vrc_ipc_stream_wait) */

#define VRC_MEM_HOST   0
#define VRC_MEM_DEVICE 1

#define VRC_MAX_DEPTH 11          /* the loop bound of lsvo.hpp:72 binds from depth 12 on */
#define VRC_MAX_NODES (1ull << 29) /* 4 GiB of LNodes: the walk addresses a node by a 32-bit byte offset */

/* include/lsvo_utils.hpp:5-18 -- the 8-byte linear octree node the kernels
 * consume: index 0 = root; a non-empty internal node i owns the 8 consecutive
 * slots starting at i + child_offset, slot k = child (x=k&1, y=k>>1&1, z=k>>2)
 * (src/lsvo_utils.cpp:29-47). */
typedef struct vrc_lnode {
    uint8_t color;
    uint8_t child_mask;
    uint8_t leaf_mask;
    uint8_t pad;
    uint32_t child_offset;
} vrc_lnode;

/* include/volumetric.hpp:7-22 (HitPoint, 48 bytes).  `const Cell* cell` is
 * replaced by `hit` + `node`: hit = kind | child_shift<<8 | scale<<16 with
 * kind 0 = miss (cell == nullptr), 1 = unit-voxel leaf (lsvo.hpp:92-95),
 * 2 = LOD cut-off (lsvo.hpp:82-85); node = index of the LNode whose child was
 * hit.  The cell is always {Solid, Grass} (lsvo.hpp:21-23).  On a miss all
 * other fields except `complexity` are zero (uninitialised in the reference). */
typedef struct vrc_hit {
    float position[3];
    float normal[3];        /* (+-1,0,0) (0,+-2,0) (0,0,+-4), lsvo.hpp:149 */
    float voxel_coord[2];
    uint32_t hit;
    uint32_t node;
    float distance;
    uint32_t complexity;    /* loop iterations, lsvo.hpp:73 */
} vrc_hit;

typedef struct vrc_scene vrc_scene;        /* device-resident LSVO + albedo tables */
typedef struct vrc_grid vrc_grid;          /* device-resident dense Grid3D */
typedef struct vrc_renderer vrc_renderer;  /* RayCaster state: framebuffer + sample accumulators */
typedef struct vrc_volume vrc_volume;      /* device-resident editable occupancy of an S^3 volume */

const char *vrc_last_error(void);
int vrc_device_count(void);                /* >= 0, or VRC_ERR_NO_DEVICE */

/* ---- scene: LSVO<N> (lsvo.hpp:12-24) ---------------------------------- */

/* Copies `n_nodes` LNodes (host memory) to `device` and keeps them resident.
 * Replaces LSVO(const SVO<N>&) + compileSVO for a pre-compiled array.  The array
 * is checked once, on the device: every non-leaf child's 8-slot block must lie
 * inside the array, the tree must not be deeper than `depth` levels (children of
 * level depth-1 nodes are unit-voxel leaves, lsvo.hpp:90-95), and no node may be
 * reachable at two different levels; a malformed or truncated array is
 * VRC_ERR_INVALID, never an out-of-bounds read in the walk. */
int vrc_scene_create(const vrc_lnode *lnodes, uint64_t n_nodes, uint32_t depth,
                     int device, vrc_scene **out);
/* 16x16 RGB tables, top-down rows, as sf::Image::getPixel sees
 * res/grass_{top,side}_16x16.bmp (raycaster.hpp:53-54). */
int vrc_scene_set_textures(vrc_scene *s, const uint8_t top_rgb[768], const uint8_t side_rgb[768]);
int vrc_scene_destroy(vrc_scene *s);
uint64_t vrc_scene_node_count(const vrc_scene *s);
uint32_t vrc_scene_depth(const vrc_scene *s);

/* Scene construction that precedes the path (main.cpp:59-88):
 * builds the exact compileSVO layout (lsvo_utils.cpp:4-49) for the terrain
 * generator of main.cpp:63-76 from height[x*size+z] (the int32 `height` of
 * main.cpp:69), without a pointer tree.  Host code.  *out is released with
 * vrc_free_host. */
int vrc_build_terrain_lsvo(const int32_t *height, uint32_t depth,
                           vrc_lnode **out, uint64_t *n_nodes);
/* Same layout for an arbitrary occupancy volume: solid[(x*size+y)*size+z] != 0. */
int vrc_build_volume_lsvo(const uint8_t *solid, uint32_t depth,
                          vrc_lnode **out, uint64_t *n_nodes);
void vrc_free_host(void *p);

/* The same construction on the GPU, straight into HBM (no host array): dense
 * per-level count / rank sweeps, bit-identical output.  height / solid are host
 * buffers laid out as above; *build_ms (optional) receives the device time of the
 * build kernels.  vrc_scene_download_nodes copies the resident array back
 * (vrc_scene_node_count entries). */
int vrc_scene_build_terrain(const int32_t *height, uint32_t depth, int device, vrc_scene **out, float *build_ms);
int vrc_scene_build_volume(const uint8_t *solid, uint32_t depth, int device, vrc_scene **out, float *build_ms);
int vrc_scene_download_nodes(const vrc_scene *s, vrc_lnode *dst);

/* The scene generator's noise on the GPU: height[x*size + z] =
 * int32(64 * noise(0.75x, 0.75z) + 32) with the reference's FastNoise settings
 * (SimplexFractal FBM, 3 octaves, frequency 0.01; seed 1337 in main.cpp:61),
 * bit-identical to lib/fastnoise.  vrc_scene_build_fastnoise_terrain runs
 * main.cpp:59-88 end to end on the device: noise -> heights -> LSVO in HBM. */
int vrc_terrain_heights(int32_t seed, uint32_t size, int device, int32_t *height_host);
int vrc_scene_build_fastnoise_terrain(int32_t seed, uint32_t depth, int device, vrc_scene **out, float *build_ms);

/* ---- per-ray operator: Volumetric::castRay (volumetric.hpp:58, lsvo.hpp:33) */

/* Batch form of HitPoint castRay(position, direction, ray_size_coef,
 * ray_size_bias).  org_xyz / dir_xyz: n x 3 floats; coef / bias: n floats or
 * NULL (= 0).  `mem` says where ALL ray and output buffers live
 * (VRC_MEM_HOST: staged through the library, synchronous -- the staging block is kept
 * per device between calls, grow-only up to 1 GiB; VRC_MEM_DEVICE: used in place,
 * asynchronous on `stream`). */
int vrc_cast_rays(const vrc_scene *s, uint64_t n,
                  const float *org_xyz, const float *dir_xyz,
                  const float *coef, const float *bias,
                  vrc_hit *out, int mem, void *stream);

/* Chains of two casts, the way RayCaster::castRay chains them (raycaster.hpp:131 -> :153; :194 ->
 * :198): ray A as vrc_cast_rays casts it (coefficient and bias 0), then ray B -- origin next to A's
 * hit -- cast with ray_size_coef = coef_b (0 <= coef_b <= 0.5; bias 0) and STARTED BELOW THE ROOT on
 * the path A's walk left, exactly as the frame kernels start their shadow / GI / GI-shadow rays
 * (csrc/vrc_device.h: start_scale_next_to[_lod]); where A missed, B starts at the root.  out_b[i]
 * equals vrc_cast_rays of ray B alone bit for bit (complexity included: the iterations a start below
 * the root leaves out are counted, lsvo.hpp:73); not_executed[i] (may be NULL) = how many those were.
 * Device buffers only (as VRC_MEM_DEVICE above); asynchronous on `stream`. */
int vrc_cast_ray_chains(const vrc_scene *s, uint64_t n,
                        const float *org_a_xyz, const float *dir_a_xyz,
                        const float *org_b_xyz, const float *dir_b_xyz, float coef_b,
                        vrc_hit *out_a, vrc_hit *out_b, uint32_t *not_executed, void *stream);

/* Single-ray form for Camera::getClosestPoint (camera_controller.hpp:56-60). Synchronous; thread-safe
 * (calls on one scene are serialised).  Uses a pinned slot and a stream owned by the scene: no
 * allocation, no device-wide synchronisation, frames in flight on other streams are not disturbed. */
int vrc_cast_ray(const vrc_scene *s, const float org[3], const float dir[3],
                 float ray_size_coef, float ray_size_bias, vrc_hit *out);

/* ---- editable volume: Volumetric::setCell (volumetric.hpp:59; empty in LSVO, lsvo.hpp:26) ---- */

/* A scene is never patched in place: frames in flight keep reading it.  What is edited is a vrc_volume, the occupancy
 * of an S^3 volume (S = 1 << depth, depth 2..10 as for the GPU builder) resident on one device -- one byte per
 * 2 x 2 x 2 brick, 16 MiB at 512^3, 128 MiB at 1024^3 -- and vrc_volume_commit builds a NEW scene from it with the
 * builder's sweeps, bit-identical to compileSVO of the current voxel set.  Coordinates are SVO::setCell's
 * (svo.hpp:72), the ones vrc_build_volume_lsvo's solid[(x*S + y)*S + z] uses. */
int vrc_volume_create(uint32_t depth, int device, vrc_volume **out);      /* empty; albedo tables white */
/* Rasterises a resident scene's LNode[] into a new volume on the scene's device (this is what makes a scene that was
 * generated on the device editable) and copies its albedo tables.  A leaf above the unit-voxel level is solid throughout. */
int vrc_volume_from_scene(const vrc_scene *s, vrc_volume **out);
int vrc_volume_destroy(vrc_volume *v);
uint32_t vrc_volume_depth(const vrc_volume *v);
/* n voxels (n x 3 uint32: x, y, z), ALL set (solid != 0) or ALL cleared: one value per call, so the result does not
 * depend on the order in which the device applies them; duplicates are legal, coordinates outside the volume are
 * dropped (the rule for setCell).  `mem` as in vrc_cast_rays: VRC_MEM_HOST = staged,
 * synchronous; VRC_MEM_DEVICE = read in place, asynchronous on `stream`.  Successive calls are ordered by stream
 * order -- issue a volume's asynchronous edits on ONE stream (or order the streams yourself). */
int vrc_volume_set_voxels(vrc_volume *v, uint64_t n, const uint32_t *xyz, int solid, int mem, void *stream);
/* n axis-aligned boxes (n x 6 uint32: lo x y z inclusive, hi x y z exclusive), clipped to the volume; empty boxes are
 * legal.  Cost follows the bricks inside the boxes (whole 32-bit words of bricks are stored as such), not the bounding
 * volume of all of them. */
int vrc_volume_fill_boxes(vrc_volume *v, uint64_t n, const uint32_t *lo_hi, int solid, int mem, void *stream);
/* Builds a new scene from the current occupancy (after every edit issued so far, whatever its stream).  Synchronous.
 * The volume stays valid and editable; scenes committed earlier are untouched and belong to the caller, who destroys
 * them (vrc_scene_destroy) once no frame uses them any more.  The new scene carries the volume's albedo tables.
 * *build_ms (optional) as for vrc_scene_build_volume.  The volume keeps the builder's per-level grids between commits
 * (12 bytes per cell of every level: 1.8 GiB at depth 10, 230 MiB at depth 9), allocated by the first commit. */
int vrc_volume_commit(vrc_volume *v, vrc_scene **out, float *build_ms);
/* Dense copy for the host, solid_host[(x*S + y)*S + z] = 0 / 1 (S^3 bytes, the layout of vrc_build_volume_lsvo), and
 * the number of solid voxels.  Synchronous, after every edit issued so far. */
int vrc_volume_download(vrc_volume *v, uint8_t *solid_host);
int vrc_volume_solid_count(vrc_volume *v, uint64_t *count);

/* The voxel a ray hit, for "dig / build at the crosshair": pure host arithmetic, no device.  For a unit-voxel hit
 * (hit->hit & 0xff == 1) voxel[] = the solid voxel in setCell coordinates (S-1 - floor((position - 1) * S) per axis:
 * the walk sees the scene point-reflected) and, when exactly one component of the normal is
 * non-zero, neighbour[] = voxel - sign(normal): the empty cell the ray came through -- *has_neighbour = 0 (and
 * neighbour zeroed) when that cell lies outside the volume or the normal is zero (a ray that started inside a solid
 * voxel).  neighbour / has_neighbour may be NULL.  A miss or an LOD cut-off is VRC_ERR_INVALID. */
int vrc_hit_to_voxel(uint32_t depth, const vrc_hit *hit, uint32_t voxel[3], uint32_t neighbour[3], int *has_neighbour);

/* Brushes, region copies and queries: what an editor does next, without leaving the device.  `mem`, `stream`, n == 0 and
 * the one-value-per-call rule are those of vrc_volume_set_voxels; the calls that read the occupancy are ordered behind
 * the volume's last asynchronous edit.
 *
 * n spheres (n x 4 int32: centre x y z, radius r): voxel (x, y, z) is set or cleared iff
 * (x-cx)^2 + (y-cy)^2 + (z-cz)^2 <= r^2 in integers.  Centres are signed and may lie outside the volume (the sphere is
 * clipped); r == 0 is the centre voxel alone, r < 0 is empty; a sphere with a centre coordinate beyond +-2^20 or r > 2^20 is
 * dropped.  Cost follows the bricks inside each sphere's own bounding box (whole 32-bit words are stored as such).  A
 * sphere is one workgroup column: a batch of more than 4096 gets one 256-thread workgroup per sphere whatever its
 * radius, so thousands of LARGE spheres in one call each walk their bounding box on four waves. */
int vrc_volume_fill_spheres(vrc_volume *v, uint64_t n, const int32_t *centre_radius, int solid, int mem, void *stream);
/* One sphere of `radius` (0 .. 2^20) at every record of a ray batch, the centres computed on the device exactly as
 * vrc_hit_to_voxel(vrc_volume_depth(v), &hits[i], ...) computes them: solid == 0 (dig) at `voxel`, solid != 0 (build) at
 * `neighbour`.  A record vrc_hit_to_voxel refuses (miss, LOD cut-off, position outside [1, 2)^3, NaN) is skipped, and so
 * is a build at a record without a neighbour.  With VRC_MEM_DEVICE, vrc_cast_rays(..., VRC_MEM_DEVICE, stream) followed
 * by this call on the same stream edits the volume with no host copy of a hit.  The centres pass through the volume's
 * grow-only staging block (16 bytes per record). */
int vrc_volume_fill_spheres_at_hits(vrc_volume *v, uint64_t n, const vrc_hit *hits, int32_t radius, int solid, int mem, void *stream);

/* Capsules: the ball swept along a segment -- a line, a beam, a pipe, and the gapless stroke through the hits of a ray batch.
 * The largest coordinate and radius of a capsule.  With a voxel p inside a volume of at most 1024^3, |a|, |b| <= 2^13 and
 * r <= 2^13, every component of q = p - a is below 2^13 + 2^10 and of d = b - a at most 2^14, so q.q < 3 (2^13 + 2^10)^2
 * < 2^28, L2 = d.d <= 3 * 2^28 < 2^30, |t| = |q.d| <= sqrt(q.q L2) < 2^29, and each product of the rule below -- (q.q) L2,
 * t^2, r^2 L2 -- stays below 2^58: the rule is exact in 64-bit integers. */
#define VRC_STROKE_LIMIT 8192
/* n capsules (n x 8 int32: ax ay az bx by bz r reserved), in setCell coordinates, signed, possibly outside the volume (the
 * capsule is clipped).  With d = b - a, L2 = d.d, q = p - a and t = q.d, voxel p = (x, y, z) is set or cleared iff, in
 * 64-bit integers,
 *   L2 == 0 or t <= 0:   q.q <= r^2                  (the ball at a)
 *   t >= L2:             |p - b|^2 <= r^2            (the ball at b)
 *   otherwise:           (q.q) L2 - t^2 <= r^2 L2    (within r of the line, between the ends)
 * The set is the same with a and b swapped, and convex.  a == b is the sphere of vrc_volume_fill_spheres; r == 0 is the
 * lattice points on the segment; r < 0 is empty.  An item with a coordinate beyond +-VRC_STROKE_LIMIT, with
 * r > VRC_STROKE_LIMIT or with reserved != 0 is dropped.  `mem`, `stream`, n == 0, the one-value-per-call rule and the
 * ordering are those of vrc_volume_fill_spheres.  Cost follows the capsule, not its bounding box: it is cut into pieces of
 * 16 voxels along the axis in which it is longest and only the box around each piece is visited (a radius-3 diagonal of
 * 512^3 visits 1/243 of the words of its bounding box).  A capsule is one workgroup column, as a sphere is. */
int vrc_stroke_fill_capsules(vrc_volume *v, uint64_t n, const int32_t *items, int solid, int mem, void *stream);
/* The stroke through the records of a ray batch: the centres c_i exactly as vrc_volume_fill_spheres_at_hits computes them
 * (dig at `voxel`, build at `neighbour`; a record vrc_hit_to_voxel refuses, and a build without a neighbour, is no centre).
 * Item i is the capsule (c_i, c_i+1, radius) where records i and i + 1 both give a centre and max_gap == 0 or
 * |c_i+1 - c_i|^2 <= max_gap^2; the ball at c_i where record i gives a centre but that link does not hold; nothing
 * otherwise.  The result is the union of the balls at all centres and of all links: successive hits further apart than the
 * radius leave one tunnel, not a string of cavities.  A miss, an LOD cut-off or a build without a neighbour breaks the
 * stroke there, and so does a step longer than max_gap voxels (the crosshair went from a near hill to a far one).  `radius`
 * 0 .. 2^13.  Staging and ordering are those of vrc_volume_fill_spheres_at_hits (16 bytes per record in the volume's
 * staging block; no list of capsules is written): with VRC_MEM_DEVICE, vrc_cast_rays(..., VRC_MEM_DEVICE, stream) followed
 * by this call on the same stream makes no host copy. */
int vrc_stroke_fill_at_hits(vrc_volume *v, uint64_t n, const vrc_hit *hits, int32_t radius, uint32_t max_gap, int solid, int mem,
                            void *stream);
/* Solid voxelisation of a triangle mesh by crossing parity along z: bringing a model in without leaving the device.
 * n triangles (n x 9 int32: ax ay az bx by bz cx cy cz) in setCell coordinates with VRC_MESH_FRAC_BITS fractional bits, 64
 * units per voxel: the centre of voxel (x, y, z) is (64x + 32, 64y + 32, 64z + 32).  `mem`, `stream` and n == 0 as for
 * vrc_volume_fill_spheres; the call is always ordered behind the volume's last asynchronous edit.  Per triangle, in
 * 64-bit integers: n = (b - a) x (c - a), s = sign(n.z); a triangle with n.z == 0 contributes nothing.
 *   Cover: the triangle covers voxel column (x, y) iff for its centre p = (64x + 32, 64y + 32) and every edge P -> Q of
 *   a -> b, b -> c, c -> a, with d = s (Q - P) in xy and E = d.x (p.y - P.y) - d.y (p.x - P.x):  E > 0, or E == 0 and
 *   (d.y > 0 or (d.y == 0 and d.x < 0)).  A centre on an edge shared by two triangles on opposite sides of it in projection
 *   belongs to exactly one of them; on a silhouette edge to both or to neither.
 *   Flip: in a covered column voxel z is flipped iff s n . (centre - a) < 0, its centre strictly on the -z side of the
 *   plane: the prefix [0, k) of the column, k = clamp(ceil(N / (64 |n.z|)), 0, S) with
 *   N = |n.z| (a.z - 32) - s (n.x (p.x - a.x) + n.y (p.y - a.y)).
 * A voxel's state afterwards is its state on entry XOR the parity of its flips over all triangles of the call.  For a
 * closed mesh in an empty volume that is exactly the set of voxel centres inside the mesh, whatever the triangles' order
 * or winding; an open mesh is legal and fills everything under the sheet; the same mesh twice restores the volume.  The
 * result is unique: integers and XOR, no dependence on scheduling.  Columns and prefixes are clipped to the volume: what
 * lies outside is neither read nor written.  A triangle with any coordinate beyond +-2^17 units (+-2048 voxels) is
 * dropped like an out-of-range sphere (inside that range every quantity above stays below 2^57) -- and dropping ONE
 * triangle of a closed mesh breaks its parity: the columns under it come out inverted below the mesh, so keep a mesh
 * inside the range as a whole.  Cost: one atomic per triangle and covered column, then one pass over the volume's words
 * HOWEVER SMALL the mesh (a read of 16 MiB at 512^3, 128 MiB at 1024^3: voxelise a small model into a small volume and
 * vrc_volume_copy_region it into the world, or vrc_volume_stamp_affine it there turned and resized);
 * few triangles are spread over up to 1024 workgroups each, a batch of more than 4096 gets one 256-thread workgroup per
 * triangle whatever its size.  The volume keeps a scratch block of the occupancy's own size (one byte per brick: 16 MiB
 * at 512^3, 128 MiB at 1024^3), allocated by the first call and never grown or shrunk. */
#define VRC_MESH_FRAC_BITS 6
int vrc_volume_xor_mesh(vrc_volume *v, uint64_t n_tris, const int32_t *tris, int mem, void *stream);
/* Surface voxelisation of a triangle mesh (the surface half of Schwarz & Seidel 2010): the voxels a mesh TOUCHES, for a mesh
 * that has no inside -- a sail, a terrain sheet, a wall quad, a collision proxy, a model's skin -- or whose parity is broken (a
 * dropped or doubled triangle, self-intersection).  `tris` in vrc_volume_xor_mesh's format and units: n x 9 int32, 64 units per
 * voxel; voxel p occupies the closed cube [64p, 64p + 64]^3 and its centre is 64p + 32.  A triangle with a coordinate beyond
 * +-2^17 is dropped, as there.  `solid`, `mem`, `stream`, n == 0, the count limit and the ordering are those of
 * vrc_volume_fill_spheres.  One value per call -- all selected voxels are set, or all are cleared -- so the result does not
 * depend on scheduling, on the triangles' order or on duplicates.  Everything is clipped to the volume.  The call needs no scratch
 * block (vrc_volume_edit_scratch_bytes is unchanged by it).  All quantities are 64-bit integers; with |coordinate| <= 2^17 each
 * stays below 2^57.  Write A, B, C for the vertices and n = (B - A) x (C - A).
 *
 * VRC_RASTER_TOUCHED: voxel p is selected iff its closed cube and the closed triangle share a point.  Both sets are convex, so
 * that is the separating-axis test over 13 axes with non-strict inequalities: with o = 64p, for an axis L the cube's interval is
 * L.o + [64 sum_i min(L_i, 0), 64 sum_i max(L_i, 0)] and the triangle's is [min, max] of L.A, L.B, L.C, and p is selected iff the
 * two overlap (touching counts) for every L among the three unit axes, n, and the nine axes e_a x (Q - P) for the edges P -> Q of
 * A -> B, B -> C, C -> A and the unit axes e_a.  A zero axis separates nothing.  Without special cases: a triangle with n = 0 is
 * a segment or a point and selects exactly the voxels it touches (a supercover line); a triangle that lies in a voxel-boundary
 * plane selects the voxels on both sides of it.  The set is the same for any permutation of the vertices.
 *
 * VRC_RASTER_THIN: the union over the three axes a and all triangles of the following.  With (u, v) = ((a + 1) % 3, (a + 2) % 3),
 * a triangle with n_a == 0 contributes nothing on axis a; otherwise s = sign(n_a), and
 *   Cover: the triangle covers voxel column (p_u, p_v) iff its projection along a covers the centre (64 p_u + 32, 64 p_v + 32),
 *   by exactly vrc_volume_xor_mesh's Cover rule with (x, y, z) replaced by (u, v, a): the same edge functions with d = s (Q - P)
 *   and the same tie rule.
 *   Select: in a covered column, with c the centre, M = |n_a| A_a - s (n_u (c_u - A_u) + n_v (c_v - A_v)), the voxel
 *   p_a = floor(M / (64 |n_a|)) is selected if it lies in the volume: the voxel that holds the point where the column's centre
 *   line meets the plane, a crossing on a voxel boundary going to the upper voxel.  For a = z, M is xor_mesh's N + 32 |n_z|.
 * Theorem: take a triangle and a column it covers along axis a, and let c and c + 1 be the two voxels along a between which
 * vrc_volume_xor_mesh (read along a) changes state on account of that triangle: the THIN voxel of that column is c or c + 1
 * (xor_mesh's k = ceil((t - 32) / 64) for the crossing at t = M / |n_a|, the THIN voxel is floor(t / 64): k where t mod 64 <= 32,
 * k - 1 otherwise).  So two face-adjacent voxels on opposite sides of a closed mesh are never both unselected: the thin shell
 * stops a face-connected flood, and flooding the empty medium from outside it gives a solid that no doubled triangle inverts
 * (VoxelVolume.solidFromShell).  THIN is a subset of TOUCHED.
 *
 * Cost follows the surface, not the triangle's bounding box.  THIN walks, per axis, the columns of the projected bounding box:
 * one atomic per covered column.  TOUCHED walks the columns of the projection along the axis in which |n| is largest; a column
 * leaves on the three edge axes of that projection, and the plane leaves it an interval of at most five voxels, each held to the
 * 13 axes.  One triangle corner to corner of 512^3, (0,0,0) (S,S,0) (S,0,S) in voxels: the predicate is applied to 524 287
 * voxels, 524 287 are selected, the bounding box holds 134 217 728 (256 times as many).  Few triangles are spread over up to 1024 workgroups each, a
 * batch of more than 4096 gets one 256-thread workgroup per triangle whatever its size.  Measured at 512^3 on the MI355X
 * (tools/bench_raster.py, device time, the call that sets plus the call that clears, median of 5): the terrain's closed
 * merged-rectangle mesh, 583 244 triangles, TOUCHED 37.6 ms and THIN 2.02 ms next to 1.02 ms for vrc_volume_xor_mesh twice; the
 * corner-to-corner triangle TOUCHED 0.272 ms and THIN 0.044 ms next to 0.052 ms for vrc_volume_fill_boxes of its bounding box;
 * 100 000 unit-face triangles TOUCHED 5.46 ms and THIN 0.49 ms next to 0.184 ms for vrc_volume_xor_mesh twice.  TOUCHED costs
 * about 30 ns per triangle of a large batch however small the triangle: 5 to 37 times its yardsticks. */
#define VRC_RASTER_TOUCHED 0   /* every voxel whose closed cube meets the closed triangle */
#define VRC_RASTER_THIN    1   /* the voxel that holds each crossing of a voxel-centre line */
int vrc_raster_mesh(vrc_volume *v, uint64_t n_tris, const int32_t *tris, int mode, int solid, int mem, void *stream);
/* The exposed faces of the voxel set as a mesh: getting the world out without a dense download, and the inverse of
 * vrc_volume_xor_mesh.  In integers: face d = 2 * axis + side of the SOLID voxel c = (x, y, z) (side 0 = towards -axis,
 * 1 = towards +axis) is exposed iff the voxel c -/+ e_axis is empty.  A neighbour outside the volume counts as empty when
 * closed != 0 -- the mesh is then closed, and vrc_volume_xor_mesh of its triangles into an empty volume of the same depth
 * gives the voxel set back bit for bit -- and as solid when closed == 0: no faces on the volume's own faces (a terrain
 * export).
 *   Order: with n = S / 2, B = ((x>>1) n + (y>>1)) n + (z>>1) the voxel's brick and key = 8 B + (z&1) 4 + (y&1) 2 + (x&1)
 *   its bit position in the occupancy, the faces are ordered by (key >> 5, d, key & 31): by 32-bit occupancy word, then
 *   direction, then bit.  The output is unique, and a window addresses it.
 *   Window: with T the total number of faces, the call writes those of [first, first + capacity) that lie in [0, T), in
 *   that order, to out[0 ..], and touches nothing beyond what it writes; *total (may be NULL) receives T.  capacity == 0 with out == NULL is
 *   legal and gives T alone; first >= T writes nothing.  All counts are in faces.
 *   VRC_SURFACE_FACES: one record of 4 uint32 per face, x y z d.  VRC_SURFACE_TRIANGLES: two triangles per face, 2 x 9
 *   int32 in vrc_volume_xor_mesh's units (64 per voxel); face i is triangles 2i and 2i + 1.  With a = d >> 1, s = d & 1,
 *   u = (a + 1) % 3, v = (a + 2) % 3 every corner has coordinate a = 64 (c_a + s), and in (u, v) the corners are
 *   q0 = 64 (c_u, c_v), q1 = 64 (c_u + 1, c_v), q2 = 64 (c_u + 1, c_v + 1), q3 = 64 (c_u, c_v + 1); s == 1 gives
 *   (q0 q1 q2), (q0 q2 q3), s == 0 gives (q0 q2 q1), (q0 q3 q2): counter-clockwise seen from outside, the normal points
 *   out of the solid voxel.  Coordinates are <= 2^16, inside vrc_volume_xor_mesh's range.
 * `mem` says where out AND total live.  VRC_MEM_HOST: synchronous, staged in internal windows of at most 2^20 faces, so
 * the staging block never grows beyond 72 MiB on account of this call whatever the capacity.  VRC_MEM_DEVICE:
 * asynchronous on `stream`, total is a device uint64_t written in stream order; out must be 16-byte aligned for face
 * records and 4-byte aligned for triangles (8-byte alignment gets wider stores).  Both calls only read the occupancy and
 * are ordered behind the volume's last asynchronous edit; a device-memory extraction is itself recorded as the last
 * asynchronous edit, because the offsets block below is shared by every call.  vrc_volume_surface_count is synchronous:
 * counts[d] = exposed faces of direction d, their sum is T.
 * Cost: three passes on one stream -- count per workgroup of 256 words, a scan of the workgroup totals, emit -- each one
 * read of the occupancy and its neighbour words, HOWEVER SMALL the window; the writes follow the window, and a
 * workgroup whose faces miss the window leaves at once.  vrc_volume_surface_count is the first pass alone.  The volume
 * keeps a block of one 64-bit offset per workgroup plus seven totals, 8 * (ceil(words / 256) + 7) bytes: 1/128 of the
 * occupancy + 56 bytes from depth 5 up (1 MiB at depth 10, 128 KiB at depth 9), 64 bytes below; allocated by the first of
 * the two calls, never grown, counted by vrc_volume_edit_scratch_bytes.  Times: profiles/edit/bench_surface.json (512^3 terrain, 0.92 M
 * faces, MI355X: all face records in 0.09 ms, all triangles in 0.20 ms, next to 0.03 ms for vrc_volume_solid_count). */
#define VRC_FACE_XN 0   /* d = 2*axis + side; side 0 = the face towards -axis, 1 = towards +axis */
#define VRC_FACE_XP 1
#define VRC_FACE_YN 2
#define VRC_FACE_YP 3
#define VRC_FACE_ZN 4
#define VRC_FACE_ZP 5
#define VRC_SURFACE_FACES     0   /* one record per face:  4 uint32  x y z d  (the SOLID voxel, setCell coordinates) */
#define VRC_SURFACE_TRIANGLES 1   /* two triangles per face: 2 x 9 int32 in vrc_volume_xor_mesh's units (64 per voxel) */
int vrc_volume_surface_count(vrc_volume *v, int closed, uint64_t counts[6]);
int vrc_volume_extract_surface(vrc_volume *v, int closed, int format, uint64_t first, uint64_t capacity,
                               void *out, uint64_t *total, int mem, void *stream);
/* The same surface with coplanar faces merged into rectangles: what an exporter, an OBJ writer or a physics engine wants,
 * fewer records than faces (3.2 times fewer on the 512^3 terrain, 1.5 times on a dense random field, 6 for any box).  The rule is exact in integers, free of any sweep order and has a unique result.
 * The faces are vrc_volume_extract_surface's, `closed` included.  For direction d with axis a call the other two axes
 * s < r: s the stack axis, r the run axis (a = x: s = y, r = z; a = y: s = x, r = z; a = z: s = x, r = y).  A row is the set
 * of cells of one (d, c_a, c_s), indexed by c_r.  A run [r0, r1) is a maximal set of consecutive c_r of a row whose face d
 * is exposed.  A rectangle is a maximal set of consecutive rows c_s = s0 .. s0 + ns - 1 of one plane (d, c_a) that all hold
 * the IDENTICAL run [r0, r1), maximal in each of them (a row whose run contains or overlaps it does not join): a run starts
 * a rectangle iff row c_s - 1 does not hold the identical run, and its height is the number of following rows that do.
 * Every exposed face lies in exactly one rectangle and a rectangle holds exposed faces of one direction and plane only.
 * This is deliberately not greedy meshing, which cuts runs and depends on the order of its sweep.
 *   Order: by (d, c_a, s0, r0), lexicographically; it does not depend on the brick layout.  The window [first, first +
 *   capacity) addresses it exactly as vrc_volume_extract_surface's addresses the faces, with R the total number of rectangles
 *   in *total; all counts are in rectangles.  capacity == 0 with out == NULL is legal and gives R alone.
 *   VRC_SURFACE_FACES: one record of 4 uint32 per rectangle, x y z and d | (nr - 1) << 8 | (ns - 1) << 20, with (x, y, z)
 *   the rectangle's voxel of smallest coordinates, nr = r1 - r0 its extent along r and ns along s, both 1 .. 1024; the
 *   record of a 1 x 1 rectangle is its face record.  VRC_SURFACE_TRIANGLES: two triangles per rectangle, 2 x 9 int32 in
 *   vrc_volume_xor_mesh's units: the corner rule above with the extents e_a = 1, e_r = nr, e_s = ns, that is
 *   q0 = 64 (c_u, c_v), q1 = 64 (c_u + e_u, c_v), q2 = 64 (c_u + e_u, c_v + e_v), q3 = 64 (c_u, c_v + e_v), the same
 *   winding.  All corners are multiples of 64 and voxel centres lie at + 32, so the T-junctions between rectangles of
 *   different sizes do not disturb the crossing parity: vrc_volume_xor_mesh of the closed mesh into an empty volume of the
 *   same depth gives the voxel set back bit for bit.
 * `mem`, `stream`, the alignment of a device buffer (16 bytes for records, 4 for triangles, 8 gets the wide stores; a
 * misaligned buffer is refused and not written), the internal windows of 2^20 records of the host form and the ordering are
 * vrc_volume_extract_surface's: both calls only read the occupancy, are ordered behind the volume's last asynchronous edit,
 * and a device-memory extraction is itself recorded as the last asynchronous edit because the block below is shared.
 * vrc_rect_count is synchronous: counts[d] = rectangles of direction d, their sum is R.  Depths 2 .. 10.
 * Cost (csrc/vrc_rects.hip): the brick words are first turned into two dense row bit fields, Z-rows [x][y][z bits] and
 * Y-rows [x][z][y bits], where the faces of a row are row & ~(the same row of the plane beside it); then count, scan and
 * emit as for the faces, one lane per 32-bit word of a row: the run starts of a word are m & ~(m << 1 | carry), each is
 * followed to its end and tested against the row before, and the emit pass walks the rows after a start for the height.
 * Every call reads the whole occupancy and rebuilds both row fields HOWEVER SMALL the window, capacity == 0 included, and
 * the scan of the workgroup offsets is one workgroup walking the slots 1024 at a time: 96 steps at depth 9, 768 serial
 * steps at depth 10.  The volume keeps one block for it: with S = 2^depth,
 * w = max(1, S / 32) and L = 6 S^2 w,  8 * (ceil(L / 256) + 7) + 8 S^2 w  bytes -- the offsets and totals, then the two
 * row fields (S^3 / 4 bytes from depth 5 up): 32.75 MiB + 56 bytes at depth 9, 262 MiB + 56 at depth 10; allocated by the
 * first of the two calls, never grown, counted by vrc_volume_edit_scratch_bytes from then on.
 * Times: profiles/edit/bench_rects.json (tools/bench_edit.py --rects; 512^3, MI355X, next to the surface calls in the same
 * run): the terrain, 0.92 M faces in 0.29 M rectangles (T / R = 3.17) -- count 0.47 ms, all records 1.97 ms, all triangles
 * 2.11 ms, next to 0.15 / 0.09 / 0.20 ms for the faces; a dense random 128^3 field, T / R = 1.50 -- 0.36 / 0.52 / 0.58 ms
 * next to 0.12 / 0.07 / 0.20.  Fewer records and bytes, but MORE time than the face calls, 3 to 22 times: as a
 * faster export this first version does not deliver.  The passes have not been timed apart.  From the code the likely
 * costs are the rebuild of the row fields by every call, six lanes per row word where the faces take one lane per
 * occupancy word, and the emit pass, where ONE lane follows a run to its end and walks the rows after it for the height --
 * 511 rows of 16 words under the terrain's 512 x 512 floor rectangle. */
int vrc_rect_count(vrc_volume *v, int closed, uint64_t counts[6]);
int vrc_extract_rects(vrc_volume *v, int closed, int format, uint64_t first, uint64_t capacity,
                             void *out, uint64_t *total, int mem, void *stream);
/* The solid voxels as a coordinate list: the inverse of vrc_volume_set_voxels, and the answer to "which voxels are solid
 * here?" without a dense download -- voxels drawn as instances, a particle per voxel of the debris, a .vox-style export, a
 * host-side rule over the surface voxels only.  With VRC_VOXELS_NEIGHBOURS every voxel brings what is around it, which is
 * what per-vertex ambient occlusion and smooth normals are computed from.  All in integers.
 *   Neighbourhood mask: bit k = 9 (dx + 1) + 3 (dy + 1) + (dz + 1) of m is set iff voxel c + (dx, dy, dz) is solid, for
 *   dx, dy, dz in {-1, 0, 1}.  Bit 13, the voxel itself, is therefore always set; bits 27 .. 31 are 0.  A neighbour outside
 *   the volume reads empty when closed != 0 and solid when closed == 0: the surface call's rule.  The six face neighbours
 *   are bits 4 (-x), 22 (+x), 10 (-y), 16 (+y), 12 (-z) and 14 (+z).
 *   which: VRC_VOXELS_ALL, every solid voxel; VRC_VOXELS_SURFACE, the solid voxels with at least one of those six bits
 *   clear; VRC_VOXELS_INTERIOR, those with all six set.  This holds for both formats, so `closed` matters to SURFACE and
 *   INTERIOR even with VRC_VOXELS_XYZ.  The cleared face bits over the SURFACE voxels of the whole volume are exactly the
 *   faces of vrc_volume_surface_count with the same `closed`.
 *   Box: lo_hi is vrc_volume_fill_boxes' form, lo inclusive, hi exclusive, clipped to the volume; NULL is the whole
 *   volume, and an empty box is legal and gives 0.  The box only selects which voxels are listed: their neighbours
 *   outside the box but inside the volume read their true value.
 *   Order: ascending key, key = 8 B + (z&1) 4 + (y&1) 2 + (x&1) with B the voxel's brick index ((x>>1) n + (y>>1)) n +
 *   (z>>1), n = S / 2: the key of the surface order and of the component representatives.  The output is unique, and a
 *   window addresses it.
 *   Window: with T the total number of voxels, the call writes those of [first, first + capacity) that lie in [0, T), in
 *   that order, to out[0 ..], and touches nothing beyond what it writes; *total (may be NULL) receives T.  capacity == 0
 *   with out == NULL is legal and gives T alone; first >= T writes nothing.  All counts are in voxels.
 *   VRC_VOXELS_XYZ: 3 uint32 per voxel, x y z -- vrc_volume_set_voxels' input form, so a list extracted into device
 *   memory goes straight back into a volume on the same stream.  VRC_VOXELS_NEIGHBOURS: 4 uint32 per voxel, x y z m.
 * `mem` says where out AND total live.  VRC_MEM_HOST: synchronous, staged in internal windows of at most 2^20 records,
 * so the staging block never grows beyond 16 MiB on account of this call whatever the capacity.  VRC_MEM_DEVICE:
 * asynchronous on `stream`, total is a device uint64_t written in stream order; out must be 16-byte aligned for
 * VRC_VOXELS_NEIGHBOURS and 4-byte aligned for VRC_VOXELS_XYZ; a misaligned buffer is refused and not written.  The
 * calls only read the occupancy and are ordered behind the volume's last asynchronous edit; a device-memory extraction
 * is itself recorded as the last asynchronous edit, because the offsets block is shared.  vrc_voxels_count is
 * synchronous and equals *total of vrc_voxels_extract with the same arguments.  NULL handles, an unknown which, format
 * or mem, out == NULL with capacity > 0 and a misaligned device buffer are VRC_ERR_INVALID, refused before any device
 * call.  Depths 2 .. 10.
 * Cost (csrc/vrc_voxels.hip): the three passes of vrc_volume_extract_surface -- count per workgroup of 256 words, a scan
 * of the workgroup totals, emit -- HOWEVER SMALL the window; ALL reads the occupancy alone, SURFACE and INTERIOR also
 * the six neighbour words of every word in the box, and the emit pass of VRC_VOXELS_NEIGHBOURS loads the 27 words
 * around a word once per word that has a listed voxel, never once per voxel.  A word outside the box is not loaded.
 * The calls use the surface calls' offsets block (the same slots: 8 * (ceil(words / 256) + 7) bytes, allocated by the
 * first call of either family, never grown), so vrc_volume_edit_scratch_bytes stays what that section says.
 * Times: profiles/edit/voxels_timing.json (tools/bench_voxels.py; 512^3, MI355X, device time by events, median of 5, the
 * yardsticks in the same rounds).  The FastNoise terrain, 8.58 M solid voxels of which 0.65 M are surface voxels with 0.92 M
 * faces: count of ALL 0.085 ms and of SURFACE 0.092 ms (synchronous calls: the read-back is in the figure), ALL / XYZ
 * 0.453 ms (103 MB), SURFACE / XYZ 0.103 ms (7.8 MB), SURFACE / NEIGHBOURS 0.143 ms (10.4 MB), next to 0.045 ms for
 * vrc_volume_solid_count, 0.097 ms for all face records of vrc_volume_extract_surface (14.8 MB) and 8.3 ms for
 * vrc_volume_download (128 MiB).  A random field of density 0.5, 67.1 M solid voxels, 66.1 M of them surface voxels, 201.7 M
 * faces: 0.064 / 0.063 ms, ALL / XYZ 0.667 ms (805 MB), SURFACE / XYZ 0.651 ms (793 MB), SURFACE / NEIGHBOURS 0.474 ms
 * (1.06 GB), next to 0.080 ms, 1.49 ms (3.2 GB) and 8.2 ms.  Every list is 12 to 80 times faster than the dense download it
 * replaces.  The extractions are SLOWER than vrc_volume_solid_count throughout (2.3 to 10 times: three passes and a list
 * against one read), the counts 1.9 and 2.1 times on the terrain and 0.8 times on the random field, the SURFACE lists on the terrain are slower than the face records (1.07 and 1.47 times, for fewer bytes),
 * and ALL / XYZ on the terrain is the slowest per byte, 0.23 TB/s against 1.2 TB/s on the random field: a lane under the
 * terrain's surface writes 32 records of 12 bytes in a row, 384 bytes from its neighbour lane's, and nothing is shuffled
 * to coalesce them.  The passes have not been timed apart. */
#define VRC_VOXELS_ALL      0   /* every solid voxel */
#define VRC_VOXELS_SURFACE  1   /* solid, and at least one of its six face neighbours is empty */
#define VRC_VOXELS_INTERIOR 2   /* solid, and all six face neighbours are solid */
#define VRC_VOXELS_XYZ        0 /* 3 uint32 per voxel: x y z -- vrc_volume_set_voxels' input form */
#define VRC_VOXELS_NEIGHBOURS 1 /* 4 uint32 per voxel: x y z m, m the 27-bit neighbourhood mask */
int vrc_voxels_count(vrc_volume *v, int which, int closed, const uint32_t *lo_hi /* 6, NULL = whole */, uint64_t *count);
int vrc_voxels_extract(vrc_volume *v, int which, int closed, const uint32_t *lo_hi, int format,
                       uint64_t first, uint64_t capacity, void *out, uint64_t *total, int mem, void *stream);
/* Voxel src_lo + d of `src` goes to dst_lo + d of `dst` for 0 <= d < size, clipped to both volumes (what falls outside
 * either is neither read nor written).  The volumes may have different depths (a 32^3 clipboard stamped into a 512^3
 * world) and must be two different volumes on one device; any voxel offset is legal.  Asynchronous on `stream`: ordered
 * behind the last asynchronous edits of both volumes, recorded as dst's last edit.  Device-memory edits do not wait for
 * that record: do not edit src OR dst on ANOTHER stream before the copy has run (a partly covered word of dst is a plain
 * read-modify-write, so such an edit of dst can be lost, and one of src may or may not be copied). */
#define VRC_COPY_REPLACE 0   /* dst = src inside the region */
#define VRC_COPY_OR      1   /* dst |= src   (paste a model, keep what is there) */
#define VRC_COPY_ANDNOT  2   /* dst &= ~src  (carve the model's shape out) */
int vrc_volume_copy_region(vrc_volume *dst, vrc_volume *src, const uint32_t src_lo[3], const uint32_t size[3],
                           const int32_t dst_lo[3], int op, void *stream);
/* Stamps `src` into `dst` through an affine map, exact in integers: the region copy turned, mirrored and resized -- a
 * clipboard rotated a quarter turn, a body of debris tumbling, a model placed at any angle and scale -- without a dense
 * download.  The map is the INVERSE map: it says where each destination voxel reads from, so every destination voxel of the
 * box is written from exactly one source voxel and a rotation leaves no holes.
 *   The map, in 64-bit integers: for every voxel p of dst in the box [dst_lo, dst_hi), clipped to dst, c = 2p + 1 is the
 *   voxel's centre in half voxels, s_a = m[3a+0] c_x + m[3a+1] c_y + m[3a+2] c_z + t_a, and q_a = s_a >> 17 (arithmetic shift:
 *   floor).  m (row-major) has VRC_AFFINE_FRAC_BITS = 16 fractional bits, t is in units of 2^-17 voxel.
 *   Writing: the source bit is src(q) when q lies in the source volume and 0 otherwise; dst(p) becomes that bit
 *   (VRC_COPY_REPLACE), is ORed with it (VRC_COPY_OR) or has it cleared (VRC_COPY_ANDNOT).  Nothing outside the clipped box
 *   is read or written.  The result is unique, and integers in numpy reproduce it bit for bit.
 *   Examples: identity is m = 65536 I, t = 0, and equals vrc_volume_copy_region of the same box.  The quarter turn
 *   q = (p_y, S-1-p_x, p_z) is m = 65536 [[0,1,0],[-1,0,0],[0,0,1]], t = (0, S << 17, 0); a signed permutation maps centres
 *   to centres, never lands on a cell boundary and is an exact bijection.  m = 2 * 65536 I halves the model by point
 *   sampling, m = 32768 I doubles it by replication.  src and dst may differ in depth.
 *   Limits: an |m| entry above 2^20 or a |t| entry above 2^40 (inside them |s| < 2^41), NULL arguments, src == dst, volumes
 *   on different devices, an unknown op and reserved != 0 are VRC_ERR_INVALID, refused before any device call.  A box that
 *   is empty or inverted on any axis is legal: a no-op that returns VRC_OK.
 * Asynchronous on `stream`, as vrc_volume_copy_region is: ordered behind the last asynchronous edits of both volumes,
 * recorded as dst's last edit, and with the same warning -- do not edit src OR dst on ANOTHER stream before the stamp has
 * run (a partly covered word of dst is a plain read-modify-write, so such an edit of dst can be lost, and one of src may or
 * may not be stamped).  No scratch: vrc_volume_edit_scratch_bytes is unchanged.
 * The device (csrc/vrc_stamp.hip) works as the region copy does, one thread per destination occupancy word (2 x 2 x 8
 * voxels) written once; the 64-bit map is evaluated once per word and its other 31 voxels follow in 32-bit running sums,
 * and a word whose source bounding box misses the source costs no load (an OR / ANDNOT word is then not touched at all).
 * Times: profiles/edit/bench_stamp.json (tools/bench_edit.py --stamp; 512^3 terrain into a second 512^3 volume, MI355X, next
 * to vrc_volume_copy_region of the same box in the same run, 0.074 ms): the identity map 0.124 ms and a quarter turn
 * 0.125 ms, 1.69 times the copy; a 30-degree turn about two axes 0.31 ms, 4.2 times; a 64^3 clipboard at scale 2 into the
 * box vrc_affine_place names 0.029 ms, next to 0.018 ms for a 128^3 region copy.
 *
 * vrc_affine_place: pure host arithmetic, no device.  The map and the destination box of the forward placement
 * x_dst = dst_pivot + scale * R * (x_src - src_pivot) in continuous voxel coordinates (voxel p occupies [p, p+1)), rot in
 * vrc_make_rotation's layout.  In doubles, rounded to nearest: m[3a+b] = rint(65536 * R[b][a] / scale) and
 * t_a = rint(131072 * src_pivot_a - sum_b m[3a+b] * 2 * dst_pivot_b) -- from the ROUNDED m, so the pivot maps to the pivot.
 * dst_lo / dst_hi: the bounding box of the forward image of the source cube [0, S_src]^3, widened by two voxels on every
 * side and clipped to the destination; lo = hi = 0 when nothing is left.  NULLs, NaN or infinite input, scale <= 0, depths
 * outside 2..10 and a result beyond the limits above (any scale below 1/16 is one) are VRC_ERR_INVALID. */
#define VRC_AFFINE_FRAC_BITS 16
typedef struct vrc_affine { int32_t m[9]; int32_t reserved; int64_t t[3]; } vrc_affine;   /* 64 bytes; m row-major, reserved = 0 */
int vrc_volume_stamp_affine(vrc_volume *dst, vrc_volume *src, const vrc_affine *map,
                            const uint32_t dst_lo[3], const uint32_t dst_hi[3], int op, void *stream);
int vrc_affine_place(const float rot[9], float scale, const float src_pivot[3], const float dst_pivot[3],
                     uint32_t src_depth, uint32_t dst_depth, vrc_affine *map, uint32_t dst_lo[3], uint32_t dst_hi[3]);
/* vrc_affine_place_box: vrc_affine_place for a part of the source -- one piece of a labelling by its record box.  The same
 * arithmetic and refusals (one body in csrc/vrc_api.cpp); the only difference is that the source cube [0, S_src]^3 is
 * replaced by the box [src_lo, src_hi] in voxel coordinates (a vrc_component's lo / hi as they are: hi is exclusive, so the
 * box is the continuous extent of the voxels).  With src_lo = 0 and src_hi = S_src the bytes are vrc_affine_place's.  There
 * is no source depth to refuse; a box with src_lo above src_hi on an axis is VRC_ERR_INVALID. */
int vrc_affine_place_box(const float rot[9], float scale, const float src_pivot[3], const float dst_pivot[3],
                         const uint32_t src_lo[3], const uint32_t src_hi[3], uint32_t dst_depth,
                         vrc_affine *map, uint32_t dst_lo[3], uint32_t dst_hi[3]);
/* A new volume with src's depth, device, occupancy (after every edit issued so far) and albedo tables: the undo
 * snapshot.  Synchronous.  The cheaper undo step is vrc_delta_diff against one shadow clone: 8 bytes per changed word. */
int vrc_volume_clone(vrc_volume *src, vrc_volume **out);
/* solid_out[i] = 0 / 1 for voxel xyz[3i..3i+2], 0 outside the volume.  counts[i] = solid voxels in box i (n x 6 uint32 as
 * for vrc_volume_fill_boxes, clipped; empty or inverted = 0), so one whole-volume box equals vrc_volume_solid_count. */
int vrc_volume_get_voxels(vrc_volume *v, uint64_t n, const uint32_t *xyz, uint8_t *solid_out, int mem, void *stream);
int vrc_volume_count_boxes(vrc_volume *v, uint64_t n, const uint32_t *lo_hi, uint64_t *counts, int mem, void *stream);
/* Device bytes the volume holds at this moment in the scratch blocks of its edit calls: the grow-only staging block of the
 * host-memory calls, vrc_volume_flood's block, vrc_volume_xor_mesh's mark field, the surface calls' offsets block, the rectangle calls' block and
 * the slots of vrc_pack_volume / vrc_unpack_volume (0 before the first call of each).  The occupancy itself and vrc_volume_commit's grids are not counted.  Pure host
 * bookkeeping, no device call. */
int vrc_volume_edit_scratch_bytes(const vrc_volume *v, uint64_t *bytes);

/* Flood fill by connectivity, on the device: which voxels hold on to the ground, which cave is enclosed, which piece lies
 * under the crosshair.  M = the voxels of `medium` that are solid (VRC_FLOOD_SOLID) or empty (VRC_FLOOD_EMPTY); the solid
 * voxels of `region` on entry are the seeds, put there with any edit call.  On return with converged == 1, `region` is
 * exactly the set of voxels of M joined to a seed in M by a chain of neighbours (sharing a face: VRC_CONNECT_FACES; a face,
 * an edge or a corner: VRC_CONNECT_ALL) that lies in M.  Seeds outside M are dropped.  The volume's faces are walls: no
 * wrap-around, and nothing beyond them counts as empty.  The result is unique: it does not depend on scheduling or on the
 * number of sweeps.  `medium` is only read; apply the result with vrc_volume_copy_region (VRC_COPY_ANDNOT removes the
 * region from a clone of the medium: what is NOT joined to the seeds).
 *
 * The device works in global sweeps over 32^3-voxel tiles, each iterated to its local fixed point; only tiles at the
 * frontier do work.  max_sweeps caps the sweeps of this call; 0 = the library's bound, 8^depth + 1: a sweep that sets no
 * voxel has read the final state everywhere and ends the flood, every sweep before it sets at least one voxel of M, and M
 * has at most 8^depth (a sweep is expected to carry the frontier across a tile; no sweep count has been measured yet).
 * If the cap comes first the call still returns VRC_OK, with converged == 0 and a valid partial result in `region`: a
 * superset of the seeds in M and a subset of the answer.  The operation is monotone, so calling again continues from
 * there, and any sequence of capped calls ends at the region one uncapped call gives.  Every call starts from the region
 * alone (no frontier is kept between calls), so the first sweep of a continuing call stages every tile that already holds
 * a region voxel before the frontier tracking takes over: a host with a frame budget pays that once per call.
 *
 * region and medium: two different volumes of one depth on one device.  Synchronous (the host decides convergence), on
 * the NULL stream, ordered behind the last asynchronous edit of both volumes and recorded as region's last edit.
 * stats (may be NULL): reached = solid voxels of region afterwards, sweeps = global sweeps issued (counters are read back
 * every few sweeps, so a few more than needed), converged.  region keeps a grow-only scratch block (tile flags and
 * counters, 384 KiB at depth 10). */
#define VRC_CONNECT_FACES 6     /* neighbours share a face */
#define VRC_CONNECT_ALL   26    /* neighbours share a face, an edge or a corner */
#define VRC_FLOOD_SOLID 0       /* travel through the solid voxels of `medium` */
#define VRC_FLOOD_EMPTY 1       /* travel through its empty voxels (caves, the air) */
typedef struct vrc_flood_stats { uint64_t reached; uint32_t sweeps; uint32_t converged; } vrc_flood_stats;
int vrc_volume_flood(vrc_volume *region, vrc_volume *medium, int connectivity, int through,
                     uint32_t max_sweeps, vrc_flood_stats *stats);

/* Connected components, on the device: every piece of M named in one call -- the debris of a dig as separate bodies, the
 * floating specks a leaky model leaves behind vrc_volume_xor_mesh, every enclosed cave (through = VRC_FLOOD_EMPTY), the
 * piece under each crosshair of a ray batch.  M is the flood's M: the solid voxels of `medium` (VRC_FLOOD_SOLID) or its
 * empty voxels (VRC_FLOOD_EMPTY); the volume's faces are walls, there is no wrap-around and nothing beyond them counts as
 * empty.  A component is a maximal subset of M whose voxels are joined by chains of neighbours lying in M; neighbours share
 * a face (VRC_CONNECT_FACES) or a face, an edge or a corner (VRC_CONNECT_ALL).
 *
 * Order and ids.  A voxel's key is the surface order's: 8 B + (z&1) 4 + (y&1) 2 + (x&1), B its brick index
 * ((x/2) n + y/2) n + z/2.  A component's representative is its voxel of minimum key, and components are numbered
 * 0 .. C-1 by ascending representative key.  The labelling is therefore unique: it depends neither on scheduling nor on
 * the number of passes, and two calls give identical bytes.
 *
 * vrc_volume_label_components is synchronous (the host needs C to size its buffers), on the NULL stream, ordered behind
 * the medium's last asynchronous edit, and only reads the medium.  Depths 2..10.  The result is a SNAPSHOT: later edits of
 * the medium do not change it, and destroying the medium leaves it valid.  It owns its memory: 4 bytes per voxel for the
 * ids plus 48 bytes per component -- 512 MiB at 512^3, 4 GiB at 1024^3 (8^10 = 2^30 voxels: keys and ids fit 32 bits).
 * *n_components may be NULL; an empty M gives C = 0 and a valid handle.
 *
 * The device labels by union-find on the id array (csrc/vrc_components.hip): a kernel per phase on one stream, labels
 * only ever lowered with 32-bit vector atomics, no workgroup waiting for another; about eight passes over the id array.
 * No time has been measured yet (tools/bench_edit.py --components writes profiles/edit/bench_components.json).
 *
 * vrc_labels_components writes the records of [first, first + capacity) that lie in [0, C), in id order, to out[0..]
 * and touches nothing beyond what it writes; first >= C writes nothing, capacity == 0 with out == NULL is legal.
 * vrc_labels_at: ids[i] = the component of voxel xyz[3i..3i+2], VRC_NO_COMPONENT for a voxel outside M or outside the
 * volume (with vrc_hit_to_voxel: the piece under every crosshair of a ray batch).
 * vrc_labels_select: keep has C bytes; with K = { v in M : keep[id(v)] != 0 } over the whole volume, dst becomes K
 * (VRC_COPY_REPLACE), dst | K (VRC_COPY_OR) or dst & ~K (VRC_COPY_ANDNOT).  dst is a volume of the labels' depth on the
 * labels' device and may be the medium itself; C == 0 with keep == NULL is legal.  Whole words are written once with
 * plain stores.
 * mem / stream as in vrc_volume_get_voxels: VRC_MEM_HOST is staged and synchronous, VRC_MEM_DEVICE works in place and is
 * asynchronous on `stream`; a device-memory select is recorded as dst's last asynchronous edit, as vrc_volume_copy_region
 * is.  NULL handles, a connectivity other than 6 / 26, a `through` other than 0 / 1, an unknown op, a depth or device
 * mismatch and a bad `mem` are VRC_ERR_INVALID, refused before any device call. */
typedef struct vrc_labels vrc_labels;    /* a snapshot: the component id of every voxel of M, resident on the volume's device */
#define VRC_NO_COMPONENT 0xffffffffu
typedef struct vrc_component {           /* 48 bytes */
    uint32_t first[3];                   /* the representative: flooding `medium` from it gives this piece back (not for vrc_fracture_label's) */
    uint32_t lo[3], hi[3];               /* bounding box, lo inclusive, hi exclusive (vrc_volume_fill_boxes' form) */
    uint32_t reserved;                   /* 0 */
    uint64_t voxels;
} vrc_component;
int vrc_volume_label_components(vrc_volume *medium, int connectivity, int through, vrc_labels **out, uint64_t *n_components);
int vrc_labels_destroy(vrc_labels *l);
uint64_t vrc_labels_count(const vrc_labels *l);
uint32_t vrc_labels_depth(const vrc_labels *l);
uint64_t vrc_labels_bytes(const vrc_labels *l);          /* device bytes held; pure host bookkeeping */
int vrc_labels_components(const vrc_labels *l, uint64_t first, uint64_t capacity, vrc_component *out, int mem, void *stream);
int vrc_labels_at(const vrc_labels *l, uint64_t n, const uint32_t *xyz, uint32_t *ids, int mem, void *stream);
int vrc_labels_select(const vrc_labels *l, const uint8_t *keep, vrc_volume *dst, int op, int mem, void *stream);

/* Loose pieces fall as rigid bodies, on the device: the step between "this piece is loose" (vrc_volume_flood,
 * vrc_volume_label_components of the debris) and "commit the new scene".  vrc_fall_drops says how far every piece of a
 * labelling can fall, vrc_fall_place writes every piece, moved by its own offset, into a volume.
 * Both work on a vrc_labels snapshot; like vrc_travel_field and vrc_travel_trace_paths on the distance snapshot they carry the
 * name of what they compute, vrc_fall_*, as their stats record vrc_fall_stats does.
 *
 * The rule, exact in integers.  `direction` is a face code d = 2*axis + side (VRC_FACE_*); the unit step is g = -e_axis for
 * side 0 and +e_axis for side 1, and "ahead of v" means v + k g, k >= 1.  Which way is down is the caller's business: the
 * terrain generator makes a column solid for y in [S/2 + 1, S/2 + lim) in setCell coordinates, so the slab the terrain stands
 * on lies towards -y, and down is VRC_FACE_YN there.  The pieces P_0 .. P_{C-1} are the components of the labels' set M,
 * whatever connectivity and `through` the labels were made with.  F is the set of solid voxels of `fixed`, a volume of the
 * labels' depth on the labels' device that is only read; NULL means empty.  The volume's faces are walls.  The drops
 * D_i >= 0 are the GREATEST integers such that for every voxel v of P_i
 *   1. v + D_i g lies inside the volume;
 *   2. D_i = 0 if v itself is in F, and D_i <= k - 1 for every f = v + k g in F with k >= 1;
 *   3. D_i <= D_j + k - 1 for every w = v + k g in P_j with j != i and k >= 1;
 *   4. D_i <= drop_limit if drop_limit != 0.
 * This is a shortest-path system with non-negative weights, so it has exactly one greatest solution, and that solution is
 * what the literal simulation gives: at every tick the largest set of pieces that can all move one cell together moves, a
 * piece being blocked if it overlaps F, touches F or the wall ahead, has reached drop_limit, or rests on a blocked piece.
 * Order within a column is preserved, so nothing passes through anything, and after the move no voxel of a piece shares a
 * cell with F or with another piece unless it already did on entry.
 *
 * vrc_fall_drops writes offsets[3i .. 3i+2] = D_i * g to host or device memory, as `mem` says; with device memory the pair
 * fall -> place needs no host copy.  It is synchronous (the host decides convergence), runs on the NULL stream and is
 * ordered behind the last asynchronous edit of `fixed`.  stats may be NULL; C == 0 is legal: zero stats, offsets untouched.
 * All scratch -- one uint32 per piece, a changed flag, the union of the pieces' boxes and the stats, plus the staged offsets
 * of a host-memory call -- is freed before return; vrc_volume_edit_scratch_bytes does not change.
 * The device (csrc/vrc_fall.hip) relaxes in rounds, one launch each: a scan of every voxel column along the direction from
 * the far face backwards carries the nearest non-empty voxel ahead (the wall, F or a piece, and its distance -- nothing
 * farther ahead can bind) and lowers D[i] with a 32-bit vector atomicMin.  Every value written is an upper bound of the
 * answer, values only decrease, and a round that lowers nothing has found every constraint satisfied: in-place relaxation
 * ends at the greatest solution whatever the schedule, and two calls give identical bytes.  The host reads a changed flag
 * after every round; the loop is bounded by C + 1 rounds and reaching the bound is an internal error (VRC_ERR_HIP), never
 * a partial result.  Along z a wave takes 64 cells of a column at a time and resolves them from ballots, along x and y a
 * lane takes a column; a wave whose lanes all lower the same piece issues one atomic; the launch covers the union of the
 * pieces' boxes extended to the far face.
 * Measured on an MI355X at 512^3 on the FastNoise terrain (tools/bench_edit.py --fall, profiles/edit/bench_fall.json; two
 * bands and a grid of cuts leave 404 loose blocks of 1.9 M voxels over 5.6 M supported ones; device time by events, median
 * of 5): the whole vrc_fall_drops call towards -y 0.57 ms in 2 rounds (largest drop 7), vrc_fall_place of all pieces
 * 0.19 ms, next to 1.93 ms of vrc_volume_label_components and 0.20 ms of vrc_labels_select of the same labels in the same
 * run -- a round, with the call's allocation, init pass and flag read-back shared out, costs 0.15 of the labelling.  The
 * rounds have not been timed apart.
 *
 * vrc_fall_place: every voxel p of M with keep[id(p)] != 0 (keep: C bytes, NULL = all) sets (VRC_COPY_OR) or clears
 * (VRC_COPY_ANDNOT) the voxel p + offsets[id(p)] of dst.  Targets outside the volume are dropped, the setCell rule; a piece
 * with an offset component beyond +-2^20 is dropped whole, like an out-of-range sphere.  The offsets are arbitrary -- a
 * fall's, or a physics engine's -- and two pieces may land on the same voxels.  VRC_COPY_REPLACE is VRC_ERR_INVALID: a
 * scatter has no unique "replace".  dst may be the labelled medium itself, because the labels are a snapshot.  The device
 * scatters with 32-bit vector atomic OR / AND on the occupancy words, the lanes of a wave that hit one word joining their
 * bits first, so the result does not depend on scheduling.  mem says where keep and offsets live: VRC_MEM_HOST is staged
 * and synchronous; VRC_MEM_DEVICE works in place and is asynchronous on `stream`, ordered behind dst's last asynchronous
 * edit and recorded as dst's last edit, with the warning of vrc_volume_copy_region: do not edit dst on ANOTHER stream
 * before the scatter has run.
 *
 * NULL `l`, `offsets` (when C > 0) or `dst`, a direction outside 0..5, a depth or device mismatch, a bad `mem` and an
 * unknown op are VRC_ERR_INVALID, refused before any device call. */
typedef struct vrc_fall_stats {          /* 32 bytes */
    uint64_t moved_voxels;               /* voxels of pieces with D > 0 */
    uint32_t pieces, moved_pieces;       /* C; pieces with D > 0 */
    uint32_t max_drop;                   /* largest D, 0 when C == 0 */
    uint32_t rounds;                     /* relaxation rounds issued */
    uint32_t reserved[2];                /* 0 */
} vrc_fall_stats;
int vrc_fall_drops(const vrc_labels *l, vrc_volume *fixed, int direction, uint32_t drop_limit,
                    int32_t *offsets /* C x 3: D_i * g */, int mem, vrc_fall_stats *stats);
int vrc_fall_place(const vrc_labels *l, const uint8_t *keep /* C bytes, NULL = all */,
                     const int32_t *offsets /* C x 3 */, vrc_volume *dst, int op, int mem, void *stream);

/* The pieces of a labelling as rigid bodies with a pose, on the device: what a physics engine needs of every piece, and what
 * it hands back (and vrc_rigid_contacts and vrc_rigid_pair_contacts, further down, the tests of a proposed pose in between).  vrc_rigid_moments gives the raw moments that mass, centre of mass and inertia tensor follow from, without
 * a dense download of the ids; vrc_rigid_place_affine writes every piece through its OWN inverse affine map -- a set of
 * debris tumbling -- in one call where vrc_labels_select and vrc_volume_stamp_affine would take a scratch volume and two
 * calls per piece.  Both work on a vrc_labels snapshot and, like vrc_fall_*, carry the name of what they serve.  Exact in
 * integers.
 *
 * vrc_rigid_moments.  With c = 2p + 1, the centre of voxel p in half voxels, the record of piece i holds n = its number of
 * voxels, s1 = the sums of c_x, c_y, c_z over them and s2 = the sums of c_x c_x, c_y c_y, c_z c_z, c_x c_y, c_x c_z, c_y c_z.
 * Nothing can overflow: at depth 10 c <= 2047 and n <= 2^30, so every sum is below 2^22 * 2^30 = 2^52 < 2^53 -- a double
 * holds each exactly.  `voxels` equals the vrc_component's.  A voxel taken as a unit cube of unit mass, the mass is n, the
 * centre of mass s1 / (2n) in continuous voxel coordinates, and with r measured from it
 * I_aa = sum(r_b^2 + r_c^2) + n/6 and I_ab = -sum(r_a r_b), where sum(r_a r_b) = (n s2_ab - s1_a s1_b) / (4n).
 * The window is vrc_labels_components': the records of [first, first + capacity) that lie in [0, C) are written in id order
 * to out[0..] and nothing beyond them is touched; first >= C writes nothing, capacity == 0 with out == NULL is legal.  The
 * call is stateless: the snapshot gains no cache and vrc_labels_bytes does not change.  VRC_MEM_HOST is staged and
 * synchronous; VRC_MEM_DEVICE zeroes and fills `out` in place, asynchronous on `stream`, with no scratch left to free.  Sums
 * of integers do not depend on their order: two calls give identical bytes.
 * The device (csrc/vrc_rigid.hip) makes ONE pass over the id array, a lane per key, and adds straight into `out` with 64-bit
 * vector atomics -- but not one per voxel and sum.  Pieces are spatially coherent, and a wave walks consecutive keys (16
 * voxels further along z every round): a wave whose 64 keys carry one id keeps
 * the ten sums in registers from round to round, the four waves of a workgroup meet in LDS, and a workgroup wholly inside a
 * piece issues ten atomics for its 8192 keys.  A wave with several ids takes a leader's id, sums the matching lanes with
 * shuffles and masks them off, four times at the most; only the lanes left after that (a checkerboard of one-voxel pieces)
 * issue their own.  Ids outside the window and voxels outside M cost no atomic.
 *
 * vrc_rigid_place_affine.  The rule is vrc_volume_stamp_affine's, per piece.  For every piece i with keep[i] != 0 (keep: C
 * bytes, NULL = all) and every voxel p of dst in box i (boxes: C x 6 uint32, lo then hi as for vrc_volume_fill_boxes,
 * clipped to dst; an empty or inverted box skips the piece; NULL = all of dst for every piece):
 * q = (m_i (2p + 1) + t_i) >> 17 exactly as there, the source bit is 1 iff q lies inside the labels' volume and id(q) == i
 * -- a voxel of another piece, or one outside M, reads 0 -- and dst(p) is ORed with the bit (VRC_COPY_OR) or has it cleared
 * (VRC_COPY_ANDNOT).  VRC_COPY_REPLACE is VRC_ERR_INVALID, as for vrc_fall_place: pieces may overlap in dst and a gather of
 * many pieces has no unique "replace".  OR and ANDNOT commute, so the result is unique whatever the overlap and the schedule,
 * and two calls give identical bytes; nothing outside the boxes changes.  dst may differ in depth from the labels, must be
 * on the labels' device, and may be the labelled medium itself, because the labels are a snapshot.  vrc_affine_place_box
 * makes map and box of a piece from a rotation, a scale and two pivots.
 * Limits and refusals are the stamp's: an |m| entry above 2^20, a |t| entry above 2^40, reserved != 0, NULL handles, NULL
 * `maps` when C > 0, a device mismatch, a bad `mem` and an unknown op are VRC_ERR_INVALID; with VRC_MEM_HOST every map is
 * checked before any device call ("piece <i>: ..." names the first bad one).  With VRC_MEM_DEVICE the host cannot read the
 * maps: a piece whose map breaks a limit is then dropped whole, like an out-of-range offset in vrc_fall_place.  C == 0 is a
 * no-op.
 * mem says where keep, maps and boxes live.  VRC_MEM_HOST is staged (one block, freed before return) and synchronous;
 * VRC_MEM_DEVICE works in place and is asynchronous on `stream`, ordered behind dst's last asynchronous edit and recorded as
 * dst's last edit, with the warning of vrc_volume_copy_region: do not edit dst on ANOTHER stream before the call has run.
 * The device form keeps no scratch at all: the launch is a 2-D grid in which blockIdx.y strides over the pieces and
 * blockIdx.x over the destination occupancy words of that piece's box, so the host never needs the boxes' sizes.
 * The device (csrc/vrc_rigid.hip) takes one thread per (piece, destination word of 2 x 2 x 8 voxels), evaluates the 64-bit
 * map once per word and lets the other 31 voxels follow in 32-bit running sums, as the stamp does.  The piece's record box
 * [lo, hi) stands in for the source volume: a word whose source bounding box misses it costs no load of ids, one wholly
 * inside drops the per-voxel tests.  Words are written with 32-bit vector atomic OR / AND, a word whose 32 bits are all 0
 * issues nothing; the lanes of a wave own different words, except in a 4^3 destination, where two brick rows share a word
 * and the lanes that hit one word join their bits first.
 * Measured on an MI355X at 512^3 on the fall benchmark's scene (tools/bench_edit.py --rigid, profiles/edit/bench_rigid.json;
 * 404 loose blocks of 1.9 M voxels, the largest 17644, over 5.6 M supported ones; device time by events, median of 5,
 * everything in device memory): vrc_rigid_moments of all pieces 0.44 ms next to 0.20 ms of vrc_labels_select in the same run,
 * 2.15 times a pass that reads the same ids and sums nothing.  The scene's waves take the uniform path, but briefly: a wave
 * walks consecutive keys, 16 voxels further along z every round, and a block is 30 voxels long, so a run of one id lasts
 * about two rounds before the wave sums its registers in 64 bits and issues ten atomics.  (With a wave's rounds 64 voxels
 * apart along z, as the labelling's passes place them, the id changed every round and the same call took 0.66 ms.)  The
 * share of the three paths has not been counted.  vrc_rigid_place_affine with pure-translation maps (the fall's offsets,
 * boxes = the moved record boxes, 0.16 M words of dst in all; the result equal to vrc_fall_place's voxel for voxel) 0.075 ms
 * next to 0.19 ms of vrc_fall_place, 0.39 times: it visits the words of the boxes and not the 134 M keys of the volume.
 * With every piece turned 30 degrees about x, then y, about its own centre of mass (boxes from vrc_affine_place_box, wider
 * by the turn and the margin: 0.74 M words) 0.078 ms.  4.5 times the words in the same time: at this size the fixed grid of
 * 40 x 404 workgroups and each one's per-piece set-up seem to set the time, not the words; that has not been measured
 * apart.  NULL boxes have not been timed: every piece then visits every word of dst. */
typedef struct vrc_piece_moments {       /* 80 bytes */
    uint64_t voxels;                     /* n */
    uint64_t s1[3];                      /* sum of c_x, c_y, c_z             with c = 2p + 1 (centres in half voxels) */
    uint64_t s2[6];                      /* sum of c_x c_x, c_y c_y, c_z c_z, c_x c_y, c_x c_z, c_y c_z */
} vrc_piece_moments;
int vrc_rigid_moments(const vrc_labels *l, uint64_t first, uint64_t capacity, vrc_piece_moments *out, int mem, void *stream);
int vrc_rigid_place_affine(const vrc_labels *l, const uint8_t *keep /* C bytes, NULL = all */,
                           const vrc_affine *maps /* C */, const uint32_t *boxes /* C x 6 lo,hi; NULL = all of dst */,
                           vrc_volume *dst, int op, int mem, void *stream);

/* vrc_rigid_contacts: the test between the two halves above.  A physics engine that proposes a pose for every piece learns
 * in one call whether that pose collides with a world, where, and which way to push: for every piece of a labelling under
 * its own affine map, the exact contact record against the volume `world`.  Without it the test is one placement into a
 * scratch volume, one AND with the world and one download per piece.  Exact in integers.
 *
 * The sets.  For piece i, A_i is exactly the set of voxels vrc_rigid_place_affine would OR into a destination of world's
 * depth with the same keep, maps and boxes: the voxels p of box i, clipped to the volume, whose source
 * q = (m_i (2p + 1) + t_i) >> 17 lies inside the labels' volume with id(q) == i.  W is the set of solid voxels of `world`,
 * and W*(p) = 1 if p is in W or p lies outside the volume -- the faces are walls, as in vrc_fall_drops, where the wall
 * blocks a piece -- and 0 otherwise.  O_i = A_i and W is the penetration.  T_i, the resting contact, is the set of voxels p
 * of A_i NOT in W that have W* = 1 at one or more of the six face neighbours p +- e_a.  The normal of a voxel is
 * n(p)_a = W*(p - e_a) - W*(p + e_a), each component in {-1, 0, 1}: it points from the solid into the open.
 * The record: posed = |A_i|; overlap = |O_i|, overlap_s1 = the sum of c = 2p + 1 over O_i (centres in half voxels, as
 * vrc_piece_moments), overlap_n = the sum of n(p) over O_i; touch, touch_s1, touch_n the same over T_i; reserved = 0.  The
 * centroid of a set is s1 / (2 count) in continuous voxel coordinates, n / |n| its mean direction to push.  Nothing
 * overflows: c <= 2047 and a set has at most 2^30 voxels, so every sum is below 2^41.  All C records are written; a piece
 * that is skipped -- keep[i] == 0, an empty or inverted box, and with VRC_MEM_DEVICE a map beyond the limits -- gets an
 * all-zero record.  Sums of integers do not depend on their order: two calls give identical bytes.
 * `world` is only read, may differ in depth from the labels and must be on the labels' device.  The labels are a snapshot, so
 * world may be the labelled medium itself -- but NOTHING is excluded then: a piece at its identity pose overlaps itself in
 * every voxel.  To test against "everything else", take the piece out first (vrc_labels_select with VRC_COPY_ANDNOT into a
 * clone) or pass the supported part alone, as vrc_fall_drops takes `fixed`.  Piece against piece is vrc_rigid_pair_contacts, further
 * down: the same record for every listed pair of posed pieces, with no volume in between.
 * Memory, ordering and refusals are vrc_rigid_place_affine's.  mem says where keep, maps, boxes and out live.  VRC_MEM_HOST
 * stages the four in one block, freed before return, and is synchronous; every map is checked before any device call
 * ("piece <i>: ..." names the first bad one).  VRC_MEM_DEVICE works in place and is asynchronous on `stream`: out is zeroed
 * and filled there.  Either way the call is ordered behind world's last asynchronous edit, as vrc_volume_count_boxes is, and
 * being no edit it is not recorded as one.  NULL l or world, NULL maps or out when C > 0, a device mismatch and a bad mem are
 * VRC_ERR_INVALID before any device call.  C == 0 is a no-op.  The call keeps no scratch: vrc_volume_edit_scratch_bytes and
 * vrc_labels_bytes do not change.
 * The device (csrc/vrc_rigid.hip) runs ONE kernel of vrc_rigid_place_affine's shape -- a 2-D grid, blockIdx.y striding over
 * the pieces, blockIdx.x over the occupancy words of a piece's box -- and the same gather: the per-piece set-up and the
 * per-word map evaluation are device functions both kernels call.  Where the placement stores a word, this one reduces it.
 * A word whose gathered bits are 0 costs nothing further -- almost every word of a generous box.  Another loads the world
 * word and builds the six "neighbour is solid" masks as whole-word operations: inside the 2 x 2 x 8 word the neighbours are
 * shifts under constant masks, across its faces they come from at most six more words (the rows cx +- 1 and cy +- 1, the
 * words before and after in the row), and a neighbour beyond the volume reads as all ones.  Counts are popcounts, normals
 * differences of popcounts, and the sums of c come from popcounts of the x and y parity planes and the three bit planes of
 * the layer number -- no loop over the bits.  A lane adds in 32 bits (at most 2^15.02 words of less than 2^16 each), the
 * wave sums in 64, the four waves meet in LDS, and the non-zero ones of the 15 sums go out as 64-bit vector atomic adds in
 * plain HIP C++: at most 15 per workgroup and piece, none from a workgroup that gathered nothing.
 * Measured on an MI355X at 512^3 on the fall benchmark's scene (tools/bench_edit.py --contacts, profiles/edit/bench_contacts.json;
 * 404 loose blocks of 1.9 M voxels over 5.6 M supported ones; device time by events, median of 5, everything in device memory,
 * the zeroing of the records included): with the fall's translation maps and the moved record boxes (0.16 M words) against
 * the supported part 0.111 ms next to 0.081 ms of vrc_rigid_place_affine with the same maps and boxes in the same run, 1.37
 * times; no piece overlaps, 266 touch.  With every piece turned 30 degrees about x, then y, about its own centre of mass
 * (0.74 M words) 0.118 ms next to 0.080 ms, 1.48 times; 148 pieces overlap.  Against the whole medium (supported part and
 * debris, so that most gathered words meet solid: 1.3 M overlapping voxels) 0.110 ms and 0.116 ms: what the world holds does
 * not show at this size.  The gather, the contact step, the reduction and the zeroing have not been timed apart; NULL boxes
 * and worlds of another depth than the labels have not been timed. */
typedef struct vrc_piece_contact {       /* 128 bytes */
    uint64_t posed;                      /* |A_i| */
    uint64_t overlap;                    /* |O_i| */
    uint64_t overlap_s1[3];              /* sum of c over O_i, c = 2p + 1 (centres in half voxels, as vrc_piece_moments) */
    int64_t  overlap_n[3];               /* sum of n(p) over O_i */
    uint64_t touch;                      /* |T_i| */
    uint64_t touch_s1[3];
    int64_t  touch_n[3];
    uint64_t reserved;                   /* 0 */
} vrc_piece_contact;
int vrc_rigid_contacts(const vrc_labels *l, const uint8_t *keep /* C bytes, NULL = all */,
                       const vrc_affine *maps /* C */, const uint32_t *boxes /* C x 6 lo,hi; NULL = all of world */,
                       vrc_volume *world, vrc_piece_contact *out /* C */, int mem, void *stream);

/* vrc_rigid_pair_contacts: posed pieces against each other, pair by pair.  vrc_rigid_contacts tests every piece against a
 * world; a pile of shards that tumble onto each other needs piece against piece, and through a world that is one scratch
 * volume, one placement of the other piece and one contact call per pair -- and the record still does not say which piece
 * was hit.  Here one call takes a list of ordered pairs and gives one vrc_piece_contact per pair.  Exact in integers.
 *
 * The sets.  S_d = 2^posed_depth voxels per axis, posed_depth in 2..10; it may differ from the labels' depth.  A_i is exactly
 * the set vrc_rigid_place_affine would OR into an empty volume of depth posed_depth with the same keep, maps and boxes (NULL
 * boxes: all of that volume).  A_i is empty for a skipped piece: keep[i] == 0, an empty or inverted box, and with
 * VRC_MEM_DEVICE a map beyond the limits.
 * The record.  out[k], for pair k = (a, b) = (pairs[2k], pairs[2k + 1]), is the record of A_a against the world W = A_b
 * WITHOUT walls: W*(p) = 1 iff p is in A_b.  A neighbour beyond the volume reads 0, and so does one beyond box b, because it
 * is not in A_b.  From that W* the fields follow as in vrc_rigid_contacts: posed = |A_a|; overlap, overlap_s1 and overlap_n
 * over A_a and A_b; touch, touch_s1 and touch_n over the voxels of A_a outside A_b with a face neighbour in A_b;
 * n(p)_a = W*(p - e_a) - W*(p + e_a) points out of b, the way to push a; reserved = 0.
 * The pair is ORDERED: a caller who wants both sides lists (a, b) and (b, a); the overlap count and overlap_s1 of the two
 * are equal, the rest is not.  a == b is legal and nothing is excluded: a piece overlaps itself in every voxel.  If a is
 * skipped the record is all zero; if only b is skipped, posed = |A_a| and the rest is zero.  Three or more pieces in one
 * voxel need no rule of their own: every listed pair sees its own two sets.  A pair may be listed more than once.
 * A piece index >= C: with VRC_MEM_HOST the call is VRC_ERR_INVALID before any device call ("pair <k>: ..." names the first
 * bad pair, next to the "piece <i>: ..." of the map check); with VRC_MEM_DEVICE that pair's record is all zero.
 * Memory, ordering and refusals are vrc_rigid_contacts', without a world to order behind.  mem says where keep, maps, boxes,
 * pairs and out live.  VRC_MEM_HOST stages the five in one block, freed before return, and is synchronous; VRC_MEM_DEVICE
 * works in place, asynchronous on `stream`: out is zeroed and filled there.  NULL l, NULL maps when C > 0, NULL pairs or out
 * when n_pairs > 0, n_pairs >= 2^32, a posed_depth outside 2..10 and a bad mem are VRC_ERR_INVALID before any device call.
 * n_pairs == 0 or C == 0 is a no-op.  The call keeps no scratch: vrc_labels_bytes and vrc_volume_edit_scratch_bytes do not
 * change.  Sums of integers do not depend on their order: two calls give identical bytes.
 * The device (csrc/vrc_rigid.hip) runs ONE kernel of vrc_rigid_contacts' shape: blockIdx.y strides over the PAIRS (at most
 * 4096 rows, the rest by stride), blockIdx.x over the occupancy words of box a, and the workgroup poses both pieces with the
 * per-piece set-up the other two kernels use.  Per word a's bits come from the common gather; almost every word of a generous
 * box stops there with 0.  A word with bits needs the "world word" of b and its six face neighbours, and these are not loads
 * but gathers of piece b through its own map -- under a mask of the bits the sums will read: a's bits and their neighbours
 * inside the word for the centre (at most 32 id loads), the facing plane of 16 for an x or y neighbour, the facing layer of 4
 * for a z neighbour, 72 for the six faces instead of 192, and nothing for a face none of a's bits lie on.  A neighbour word
 * outside box b, one whose source box misses b's record box and one beyond the volume read 0 without a load.  The seven words
 * then go through the very reduction vrc_rigid_contacts uses -- shifts under constant masks, popcounts, 32-bit lane sums,
 * 64-bit wave sums, the four waves meeting in LDS, at most 15 non-zero 64-bit vector atomic adds per workgroup and pair.  No
 * dense field of "which piece owns this voxel" is built: posed pieces may overlap, so a voxel has no single owner, and a
 * field per pair is the scratch volume this call replaces.
 * Measured on an MI355X at 512^3 on the fall benchmark's scene with every piece turned 30 degrees about x, then y, about its
 * own centre of mass (tools/bench_edit.py --pair-contacts, profiles/edit/bench_pair_contacts.json; device time by events,
 * median of 5, everything in device memory): the 404 loose blocks of 1.9 M voxels give 3688 candidate pairs, listed by
 * vrc_rigid_box_pair_count + vrc_rigid_box_pairs in 0.33 ms (both synchronous, the allocation of their scratch included);
 * vrc_rigid_pair_contacts over all of them 0.81 ms, the zeroing of the records included; 652 pairs overlap (0.11 M voxels) and 798
 * touch.  The yardstick in the same run, the documented workaround timed on a sample of 64 of the pairs -- per pair the clearing
 * of a 512^3 scratch volume, vrc_rigid_place_affine of b alone into it and vrc_rigid_contacts of a alone against it: 0.098 ms a
 * pair, 360 ms scaled to the 3688, 445 times the one call.  Not timed apart: the zeroing, the two gathers and the reduction of
 * the pair kernel; the count, scan and emit passes of the broad phase; the three steps of the workaround.
 *
 * vrc_rigid_box_pair_count / vrc_rigid_box_pairs: the broad phase, the list the narrow phase wants, made from boxes that
 * live on the device.  Every box (C x 6 uint32, lo then hi, REQUIRED: with "all of the volume" every pair is a candidate and
 * the caller knows that) is clipped to [0, S_d)^3.  A piece with keep[i] == 0 or an empty or inverted box has no pairs.  The
 * ordered pair (a, b), a != b, is a candidate iff on all three axes lo_a <= hi_b and lo_b <= hi_a (hi exclusive): box a meets
 * box b grown by one voxel, which is necessary for overlap OR touch.  The relation is symmetric and both orders are listed,
 * (a, b) ascending lexicographically.  vrc_rigid_box_pair_count gives the length of that list.  vrc_rigid_box_pairs has the
 * window of vrc_labels_components: the entries of [first, first + capacity) that exist are written from pairs[0], nothing
 * beyond them is touched, first >= count writes nothing, capacity == 0 with NULL pairs is legal.  l supplies C and the device
 * and is not otherwise read.  mem says where keep, boxes and pairs live; `count` is the caller's host memory.  Both calls run
 * on `stream` and are synchronous: they return when the work is done.  NULL l, NULL count, NULL boxes when C > 0, NULL pairs
 * with capacity > 0, a posed_depth outside 2..10, a bad mem and C > 2^20 are VRC_ERR_INVALID before any device call.
 * The device: one thread per a walks all b, so every lane of a wave reads the same box b and the table comes through
 * wave-uniform loads; the pass stores a's count, one scan turns the counts into offsets, and a second pass of the same loop
 * emits what falls into the window -- the project's count, scan, emit.  Scratch is (C + 1) x 8 bytes (and the staged boxes
 * and keep of a host-memory call), freed before return.  The cost is C^2 box tests, whatever the boxes: sensible up to some
 * ten thousand pieces (10^8 tests); beyond that a caller wants a grid or a sort, and beyond 2^20 pieces the call refuses. */
int vrc_rigid_pair_contacts(const vrc_labels *l, const uint8_t *keep /* C bytes, NULL = all */,
                            const vrc_affine *maps /* C */, const uint32_t *boxes /* C x 6 lo,hi; NULL = all of the posed volume */,
                            uint32_t posed_depth,
                            uint64_t n_pairs, const uint32_t *pairs /* n_pairs x 2: a, b */,
                            vrc_piece_contact *out /* n_pairs */, int mem, void *stream);
int vrc_rigid_box_pair_count(const vrc_labels *l, const uint8_t *keep, const uint32_t *boxes /* C x 6, required */,
                             uint32_t posed_depth, uint64_t *count, int mem, void *stream);      /* synchronous */
int vrc_rigid_box_pairs(const vrc_labels *l, const uint8_t *keep, const uint32_t *boxes, uint32_t posed_depth,
                        uint64_t first, uint64_t capacity, uint32_t *pairs /* capacity x 2 */, int mem, void *stream);

/* Voronoi fracture into labelled shards, on the device: the step BEFORE "a piece is loose".  A solid body is cut along the
 * Voronoi partition around a handful of sites (impact points), no material is removed, and the result is an ordinary
 * vrc_labels snapshot: vrc_labels_*, vrc_fall_*, vrc_rigid_moments, vrc_rigid_place_affine and vrc_rigid_contacts work on
 * the shards unchanged.  Like vrc_fall_* and vrc_rigid_* the calls carry the name of what they compute.
 *
 * The rule, exact in integers.  Sites: n sites s_0 .. s_{n-1}, three int32 voxel coordinates each.  A site outside [0, S)^3
 * is ignored (the setCell rule) but keeps its place in the numbering; duplicates are legal.
 * Cell of a voxel.  For every voxel p of the volume, cell(p) is the index i of an in-volume site that minimises
 * (|p - s_i|^2, i) lexicographically: the nearest site by squared Euclidean distance, among several nearest the lowest index.
 * cell(p) = VRC_NO_COMPONENT when no site lies in the volume, and when max_d2 != VRC_DISTANCE_NONE and that least squared
 * distance exceeds max_d2 -- the cut-off is how a caller breaks only what lies within a radius of the impact: the rest of the
 * world keeps the cell "none" and stays whole.
 * Pieces.  M is the flood's M: the solid voxels of `medium` (VRC_FLOOD_SOLID) or its empty voxels (VRC_FLOOD_EMPTY); the
 * volume's faces are walls.  A piece is a maximal subset of M whose voxels are joined by chains of neighbours (6 or 26) that
 * lie in M and all carry the same cell value.  Representative, numbering and records are those of
 * vrc_volume_label_components: the voxel of minimum key, ids ascending by representative key, first / lo / hi / voxels,
 * reserved = 0.  The result is therefore unique: two calls give identical bytes.  With no in-volume site, or with max_d2
 * below every distance, it is byte for byte that of vrc_volume_label_components.  One sentence of vrc_component does NOT hold
 * for these labels: flooding `medium` from `first` gives the whole connected body back, not this piece -- a piece ends
 * where its cell ends, not where the medium does.
 *
 * vrc_fracture_label is synchronous, on the NULL stream, ordered behind the medium's last asynchronous edit, and only reads
 * the medium.  Depths 2..10.  mem says where sites_xyz lives, as in vrc_fall_drops: host memory is staged, device memory is
 * read in place (and must be complete when the call is made).  The snapshot owns what a vrc_volume_label_components snapshot
 * owns and additionally 4 bytes per piece, the piece's cell; vrc_labels_bytes counts them.  All other scratch is freed before
 * return and vrc_volume_edit_scratch_bytes does not change: the dense cell field (4 * 8^depth bytes, as much again as the
 * ids), the site table (4 bytes per site), the labelling's counts, the staged sites of a host-memory call (12 bytes per
 * site) and, from 256^3 on, the envelope stacks of the lines in flight, sized as vrc_volume_distance_field's (up to 128^3 they
 * are in LDS, 32 KiB per workgroup).
 *
 * The device (csrc/vrc_fracture.hip): the sites scatter their indices into the dense field with a 32-bit vector atomicMin,
 * then three separable passes in the shape of the distance transform's carry the INDEX of the nearest site along z, y and
 * x -- the lower-envelope stack holds site indices, one word an entry, and the partial distance is recomputed from a table
 * of the sites' coordinates.  Ties are resolved in every pass towards the lowest index (a parabola is popped from the
 * envelope only when it is strictly above it everywhere), which composes to the rule above; the last pass applies max_d2.
 * The labelling is vrc_volume_label_components' union-find with one more condition in the merge -- two neighbours unite only
 * if their cells are equal -- and a last small kernel reads every piece's cell at its representative.  Everything is integer
 * arithmetic, every atomic a 32- or 64-bit vector atomic, no workgroup waits for another.
 * Measured on an MI355X at 512^3 on the FastNoise terrain (tools/bench_edit.py --fracture, profiles/edit/bench_fracture.json;
 * sites in device memory, device time by events, median of 5, A B A B in one run, next to vrc_volume_distance_field followed by
 * vrc_volume_label_components of the same medium, the yardstick: the same traffic plus the index): 64 sites within 48 voxels of
 * a surface point with max_d2 = 48^2 (110 pieces, 108 of them shards) 16.30 ms next to 18.18 ms, 0.90 of the yardstick; 4096
 * sites over the whole volume, no cut-off (1386 pieces) 7.09 ms next to 18.01 ms, 0.39 of it -- the terrain is ONE piece for
 * the plain labelling, whose union-find is dearest on one large tree, and thousands of small trees are cheaper than the
 * index-carrying passes are dearer.  The passes have not been timed apart.
 *
 * vrc_fracture_piece_sites: sites[k] = the cell of piece first + k, VRC_NO_COMPONENT for "none", for the pieces of
 * [first, first + capacity) that lie in [0, C); the window semantics, mem and stream of vrc_labels_components.  On labels made
 * by vrc_volume_label_components it is VRC_ERR_INVALID, as vrc_travel_trace_paths is on a Euclidean field.
 *
 * NULL `medium` / `out`, n_sites == 0, NULL sites_xyz, n_sites >= 2^32 - 1 (an index must stay below VRC_NO_COMPONENT), a
 * connectivity other than 6 / 26, a `through` other than 0 / 1 and a bad `mem` are VRC_ERR_INVALID, refused before any device
 * call. */
int vrc_fracture_label(vrc_volume *medium, int connectivity, int through,
                       uint64_t n_sites, const int32_t *sites_xyz, uint32_t max_d2, int mem,
                       vrc_labels **out, uint64_t *n_components);
int vrc_fracture_piece_sites(const vrc_labels *l, uint64_t first, uint64_t capacity,
                             uint32_t *sites /* cell of piece first+k; VRC_NO_COMPONENT for "none" */,
                             int mem, void *stream);

/* The exact squared Euclidean distance field, on the device: how far every voxel is from the surface, and with it grow /
 * shrink by r voxels (dilate, erode, open, close), hollowing a solid down to a shell, clearance queries, and a field a
 * PyTorch caller reads in place.  The feature set F is the solid voxels of `medium` (to = VRC_FLOOD_SOLID) or its empty
 * voxels (to = VRC_FLOOD_EMPTY).  With outside != 0 every integer lattice point beyond the volume's faces belongs to F as
 * well -- the "closed" reading of the surface calls: an erosion then also eats from the volume's own faces; with
 * outside == 0 the faces are walls and nothing lies beyond them.
 *
 * The field.  For every voxel p of the volume D(p) = min over q in F of (px-qx)^2 + (py-qy)^2 + (pz-qz)^2, in integers;
 * D(p) = VRC_DISTANCE_NONE when F is empty (outside == 0 and no feature voxel in the volume).  Finite values are at most
 * 3 (S-1)^2 < 2^22.  With outside != 0, D(p) = min(D_inside(p), min over the three axes a of (p_a + 1)^2 and (S - p_a)^2).
 * The result is unique: it does not depend on scheduling, and two calls give identical bytes.  It is stored densely as
 * [(x*S + y)*S + z], the layout of vrc_volume_download, so vrc_distance_data is directly an (S, S, S) uint32 tensor and
 * vrc_distance_download is one copy.
 *
 * stats (may be NULL): features = |F inside the volume|; max_d2 = the largest finite D, 0 when there is none; argmax = the
 * voxel that holds it with the smallest dense index, 0,0,0 when there is none; reserved = 0.
 *
 * vrc_volume_distance_field is synchronous, on the NULL stream, ordered behind the medium's last asynchronous edit, and
 * only reads the medium.  Depths 2..10.  The result is a SNAPSHOT: it owns its memory (4 bytes per voxel: 512 MiB at 512^3,
 * 4 GiB at 1024^3), is never written after creation, later edits of the medium do not change it, and destroying the medium
 * leaves it valid.  All scratch is freed before return: 16 bytes of stats up to 128^3, where the working stacks are in
 * LDS; from 256^3 on also min(S^2 / 64, 8 x compute units) groups x 64 lanes x S x 4 bytes of stacks for the lines in
 * flight -- 64 MiB at 256^3, 256 MiB at 512^3 and 512 MiB at 1024^3 on 256 compute units -- never proportional to the volume.
 *
 * The device runs the separable transform in place on the field (csrc/vrc_distance.hip): the z pass from the occupancy
 * bits, then a min-plus pass along y and one along x by the lower-envelope stack, exact in integers (crossovers compared
 * by cross-multiplication, no float), 2 S steps per line whatever the input; one kernel per pass on one stream, no
 * workgroup waiting for another, 64-bit vector atomics for the stats only.  No time has been measured yet
 * (tools/bench_edit.py --distance writes profiles/edit/bench_distance.json).
 *
 * vrc_distance_at: d2[i] = D at voxel xyz[3i..3i+2], VRC_DISTANCE_NONE for a coordinate outside the volume; mem / stream as
 * in vrc_labels_at (VRC_MEM_HOST is staged and synchronous, VRC_MEM_DEVICE works in place, asynchronous on `stream`).
 * vrc_distance_download: all S^3 values to host memory, synchronous.
 * vrc_distance_select: with K = { p : lo <= D(p) <= hi }, VRC_DISTANCE_NONE compared as the plain value 0xffffffff, dst
 * becomes K (VRC_COPY_REPLACE), dst | K (VRC_COPY_OR) or dst & ~K (VRC_COPY_ANDNOT).  dst is a volume of the field's depth
 * on the field's device and may be the medium itself.  Whole occupancy words are written once with plain stores, one
 * thread per word.  Asynchronous on `stream`: ordered behind dst's last asynchronous edit and recorded as dst's last edit,
 * as vrc_labels_select with device memory is.  dilate(r) = select(D_solid, 0, r^2, OR), erode(r) = select(D_empty, 0, r^2,
 * ANDNOT), hollow(t) = select(D_empty, t^2 + 1, 0xffffffff, ANDNOT): the radius rule of vrc_volume_fill_spheres.
 * NULL handles, a `to` other than 0 / 1, an unknown op, lo > hi, a depth or device mismatch and a bad `mem` are
 * VRC_ERR_INVALID, refused before any device call; a NULL handle gives vrc_distance_depth = vrc_distance_bytes = 0 and
 * vrc_distance_data = NULL. */
#define VRC_DISTANCE_NONE 0xffffffffu
typedef struct vrc_distance vrc_distance;    /* a snapshot: the squared distance of every voxel, resident on the volume's device */
typedef struct vrc_distance_stats { uint64_t features; uint32_t max_d2; uint32_t argmax[3]; uint32_t reserved; } vrc_distance_stats;
int vrc_volume_distance_field(vrc_volume *medium, int to, int outside, vrc_distance **out, vrc_distance_stats *stats);
int vrc_distance_destroy(vrc_distance *d);
uint32_t vrc_distance_depth(const vrc_distance *d);
uint64_t vrc_distance_bytes(const vrc_distance *d);            /* 4 * 8^depth; pure host bookkeeping */
const uint32_t *vrc_distance_data(const vrc_distance *d);      /* DEVICE pointer, S^3 uint32, [(x*S + y)*S + z] */
int vrc_distance_at(const vrc_distance *d, uint64_t n, const uint32_t *xyz, uint32_t *d2, int mem, void *stream);
int vrc_distance_download(const vrc_distance *d, uint32_t *d2_host);
int vrc_distance_select(const vrc_distance *d, uint32_t lo, uint32_t hi, vrc_volume *dst, int op, void *stream);

/* The travel-distance field, on the device: how many steps it takes to get from a set of seeds to every voxel THROUGH the
 * medium, round every wall -- the field under pathfinding, flow fields that steer many agents at once, "where can it get to
 * in k moves", the spread of sound or fluid.  M is the flood's M: the solid voxels of `medium` (VRC_FLOOD_SOLID) or its empty
 * voxels (VRC_FLOOD_EMPTY); the volume's faces are walls, there is no wrap-around and nothing beyond them belongs to M.
 * Neighbours are the flood's: sharing a face (VRC_CONNECT_FACES), or a face, an edge or a corner (VRC_CONNECT_ALL).  Every
 * step costs 1, a diagonal one too, and a diagonal step between two voxels of M is allowed whatever lies beside it.  The
 * seeds are the solid voxels of `seeds` that lie in M; seeds outside M are dropped.
 *
 * The field.  For p in M, T(p) = the least number of steps of a chain of neighbours lying in M from any seed to p; T = 0 at a
 * seed.  T(p) = VRC_DISTANCE_NONE when p is not in M, when no chain exists, and when step_limit != 0 and the least number
 * exceeds step_limit.  Finite values are below 8^depth <= 2^30.  The result is unique: it does not depend on scheduling,
 * tile size or sweep count, and two calls give identical bytes.  vrc_volume_flood from the same seeds gives exactly the
 * voxels with a finite value of the unlimited field.
 *
 * The result is a vrc_distance SNAPSHOT like the Euclidean field's, stored as [(x*S + y)*S + z]: it owns its 4 bytes per
 * voxel, is never written after creation, is untouched by later edits and survives the destruction of both volumes.  Every
 * vrc_distance_* accessor works on it unchanged: vrc_distance_select(d, 0, k, ...) is "reachable within k steps",
 * vrc_distance_select(d, VRC_DISTANCE_NONE, VRC_DISTANCE_NONE, ...) is "never reached".  vrc_travel_connectivity returns
 * the connectivity a travel field was made with, 6 or 26, and 0 for a Euclidean field and for NULL.
 *
 * stats (may be NULL): seeds = seed voxels that lie in M; reached = voxels with a finite value, seeds included; max_steps =
 * the largest finite value, 0 when there is none; argmax = the voxel of smallest dense index that holds it, 0,0,0 when there
 * is none; sweeps = global sweeps issued (counters are read back every few sweeps, so a few more than needed); reserved = 0.
 * An empty seed set gives an all-NONE field, a valid handle and zero stats.
 *
 * seeds and medium: one depth, 2..10, on one device; both are only read and may be the same volume.  Synchronous (the host
 * decides convergence), on the NULL stream, ordered behind the last asynchronous edit of both volumes.  All scratch -- 24
 * bytes of stats, three flag words per 16^3 tile and the sweep counters, 3 MiB at 1024^3 -- is freed before return; nothing
 * is kept on either volume and vrc_volume_edit_scratch_bytes does not change.
 *
 * The device works in global sweeps over 16^3-voxel tiles (csrc/vrc_travel.hip): a tile at the frontier stages its values
 * with a one-voxel halo in LDS and relaxes T(p) = min(T(p), 1 + min over the neighbours) to its local fixed point, LOWERING a
 * value again when a shorter route arrives later than a longer one; no workgroup waits for another.  Every value ever
 * written is the length of a real chain and values only decrease, so the fixed point is T whatever the schedule.  After k
 * sweeps every voxel with T <= k is final: the sweep loop is bounded by max T + 2 <= 8^depth + 1, by step_limit + 2 under a
 * limit, and reaching that bound is an internal error (VRC_ERR_HIP), never a partial result.  Measured on an MI355X at 512^3
 * on the FastNoise terrain (tools/bench_edit.py --travel, profiles/edit/bench_travel.json): through the air from one seed
 * 6.2 ms in 54 sweeps with 6 neighbours (742 steps at most) and 9.5 ms in 46 sweeps with 26, next to 1.5 ms and 1.4 ms of
 * vrc_volume_flood from the same seed in the same run; through the solid from the slab the terrain stands on 1.05 ms and
 * 1.43 ms in 6 sweeps, next to 0.26 ms and 0.36 ms of the flood.
 *
 * vrc_travel_trace_paths reads routes off a travel field (a Euclidean one is VRC_ERR_INVALID).  For start i, lengths[i] =
 * T(start), VRC_DISTANCE_NONE when the start lies outside the volume or T is NONE, and then nothing of row i is written.
 * Otherwise voxel k of the route goes to paths_xyz[(i*capacity + k)*3 ..] for k = 0 .. min(T, capacity - 1): voxel 0 is the
 * start, voxel k + 1 the neighbour of voxel k under the field's connectivity whose value is T - k - 1 -- among several the
 * first in ascending (dx, dy, dz) order, dx most significant, each in -1..1 (for 6 neighbours: -x, -y, -z, +z, +y, +x) --
 * and the last voxel of a full route is a seed.  Nothing beyond what is written is touched; capacity == 0 with paths_xyz ==
 * NULL is legal and returns the lengths only.  mem / stream as in vrc_distance_at.  One thread per route.
 *
 * NULL handles, a connectivity other than 6 / 26, a `through` other than 0 / 1, a depth or device mismatch, a depth outside
 * 2..10, a NULL `out` and a bad `mem` are VRC_ERR_INVALID, refused before any device call. */
typedef struct vrc_travel_stats {      /* 40 bytes */
    uint64_t seeds;        /* seed voxels that lie in M */
    uint64_t reached;      /* voxels with a finite value (seeds included) */
    uint32_t max_steps;    /* largest finite value, 0 when none */
    uint32_t argmax[3];    /* the voxel of smallest dense index that holds it; 0,0,0 when none */
    uint32_t sweeps;       /* global sweeps issued */
    uint32_t reserved;     /* 0 */
} vrc_travel_stats;
int vrc_travel_field(vrc_volume *seeds, vrc_volume *medium, int connectivity, int through,
                            uint32_t step_limit, vrc_distance **out, vrc_travel_stats *stats);
int vrc_travel_connectivity(const vrc_distance *d);          /* 6 / 26: a travel field; 0: a Euclidean field, or NULL */
int vrc_travel_trace_paths(const vrc_distance *d, uint64_t n, const uint32_t *start_xyz, uint32_t capacity,
                             uint32_t *paths_xyz, uint32_t *lengths, int mem, void *stream);

/* vrc_rigid_clearance: how far a posed piece is from colliding, and how deep it is in.  vrc_rigid_contacts says whether a
 * pose collides; a piece in free flight has the same all-zero overlap / touch whether the nearest wall is 2 voxels away or
 * 200, and `overlap` counts voxels, not the way out.  Both answers lie in a vrc_distance snapshot: the squared distance to
 * the solid (to = VRC_FLOOD_SOLID) is the clearance, the one to the open (to = VRC_FLOOD_EMPTY) the penetration depth, and a
 * travel field gives "how many steps from the seeds is each piece".  This call reads such a field at the voxels of every
 * posed piece and reduces it per piece, where the only other way is one placement into a scratch volume, one download and
 * one vrc_distance_at per piece.  Exact in integers.
 *
 * The sets.  A_i is exactly the set of voxels vrc_rigid_place_affine would OR into an empty volume of the FIELD's depth with
 * the same keep, maps and boxes -- vrc_rigid_contacts' definition, with the field's depth where that call has the world's.
 * The record is the reduction of field(p) over p in A_i: posed = |A_i|; none = the voxels whose value is VRC_DISTANCE_NONE;
 * sum = the sum of the finite values (below 2^60: a value is below 2^30, a set has at most 2^30 voxels); min_value / max_value
 * = the least / greatest finite value, VRC_DISTANCE_NONE / 0 when there is none; min_at / max_at = the voxel that holds it,
 * among several the one of smallest dense index (x*S + y)*S + z, and 0,0,0 when there is none; reserved = 0.  NONE values take
 * part in neither minimum nor maximum.  All C records are written; a piece that is skipped -- keep[i] == 0, an empty or
 * inverted box, and with VRC_MEM_DEVICE a map beyond the limits -- gets the record of the empty set: min_value =
 * VRC_DISTANCE_NONE and every other byte 0.  The ties are settled, so the result is unique: two calls give identical bytes
 * whatever the schedule.  With D the field to the solid with outside = 0, min_value = 0 says the piece overlaps, and
 * otherwise every integer translation o of the posed set with |o|^2 < min_value stays clear of the solid (the set may leave
 * the volume: vrc_rigid_contacts clips it): conservative advancement.
 * Any vrc_distance snapshot is accepted, Euclidean or travel, of depth 2..10; the labels may have another depth; the field
 * must be on the labels' device.
 * Memory, ordering and refusals are vrc_rigid_contacts', with no volume to order behind: both arguments are snapshots.  mem
 * says where keep, maps, boxes and out live.  VRC_MEM_HOST stages the four in one block, freed before return, and is
 * synchronous; every map is checked before any device call ("piece <i>: ..." names the first bad one).  VRC_MEM_DEVICE works
 * in place and is asynchronous on `stream`; while the call is in flight the records hold intermediate values.  NULL l or
 * field, NULL maps or out when C > 0, a device mismatch and a bad mem are VRC_ERR_INVALID before any device call.  C == 0 is
 * a no-op.  The call keeps no scratch: vrc_labels_bytes and vrc_volume_edit_scratch_bytes do not change.
 * The device (csrc/vrc_rigid.hip) runs one kernel of vrc_rigid_contacts' shape -- the same 2-D grid, per-piece set-up and
 * per-word gather, one copy for all -- between two small ones of one thread per record.  A lane with gathered bits walks
 * them and loads the field at each, four runs of eight consecutive values a word, into a count, a count of NONE, a 64-bit
 * sum and a packed minimum (value << 32 | index) and maximum (value << 32 | ~index), so that the voxel of smallest index
 * travels with the value.  Waves reduce by shuffles, the four waves meet in LDS, and a workgroup issues at most three 64-bit
 * vector atomic adds, one atomicMin and one atomicMax per piece, none where it gathered nothing; plain HIP C++.  The record
 * itself holds the two packed words meanwhile: the kernel before writes the identities, the kernel after decodes them in
 * place.  Measured on an MI355X at 512^3 on the fall benchmark's scene (tools/bench_edit.py --clearance,
 * profiles/edit/bench_clearance.json; 404 loose blocks of 1.9 M voxels, the Euclidean field of the 5.6 M supported voxels; device
 * time by events, median of 5, everything in device memory, A B A B with vrc_rigid_contacts against the supported part with the
 * same maps and boxes in the same run): with the fall's translation maps and the moved record boxes (0.16 M words) 0.121 ms next
 * to 0.109 ms of the contact call, 1.11 times; no piece overlaps, 252 are within one voxel.  With every piece turned 30 degrees
 * about x, then y, about its own centre of mass (0.74 M words) 0.122 ms next to 0.117 ms, 1.05 times; 148 pieces overlap.  The
 * two kernels of one thread per record, the gather, the field loads and the reduction have not been timed apart; NULL boxes,
 * travel fields and fields of another depth than the labels have not been timed. */
typedef struct vrc_piece_clearance {     /* 64 bytes */
    uint64_t posed;          /* |A_i| */
    uint64_t none;           /* voxels of A_i whose field value is VRC_DISTANCE_NONE */
    uint64_t sum;            /* sum of the finite values over A_i (< 2^60: values < 2^30, at most 2^30 voxels) */
    uint32_t min_value;      /* least finite value over A_i; VRC_DISTANCE_NONE when there is none */
    uint32_t min_at[3];      /* the voxel of smallest dense index (x*S + y)*S + z that holds it; 0,0,0 when none */
    uint32_t max_value;      /* greatest finite value over A_i; 0 when there is none */
    uint32_t max_at[3];      /* the voxel of smallest dense index that holds it; 0,0,0 when none */
    uint64_t reserved;       /* 0 */
} vrc_piece_clearance;
int vrc_rigid_clearance(const vrc_labels *l, const uint8_t *keep /* C bytes, NULL = all */,
                        const vrc_affine *maps /* C */, const uint32_t *boxes /* C x 6 lo,hi; NULL = all of the field */,
                        const vrc_distance *field, vrc_piece_clearance *out /* C */, int mem, void *stream);

/* Line of sight and visible sets by exact voxel walks over a vrc_distance snapshot: can a projectile or an agent of radius r
 * go from a to b in a straight line, and what does an eye or a point light at e see.  The snapshot holds both things such a
 * query needs: it is a copy of the occupancy (D = 0 exactly on the feature set) and it holds the free radius round every voxel.
 * Both calls take snapshots only, as vrc_rigid_clearance does: they order behind nothing.  Exact in integers.
 *
 * The walk from voxel a to voxel b, both inside the volume.  The segment runs from the centre of a to the centre of b; with
 * n_c = |b_c - a_c| per axis, crossing k of axis c (k = 1..n_c) happens at t = (2k - 1) / (2 n_c).  Times are compared by
 * cross-multiplication in integers, (2k - 1) n_d against (2j - 1) n_c, products below 2^22; no float is used anywhere.  Centres
 * are half-integers, so the segment never lies in a face plane and ties are isolated points where it passes through an edge or
 * a corner.  VRC_SIGHT_THIN (flags bit 0 clear): crossings of equal t are ONE diagonal step; the visited voxels are exactly
 * those whose open cube the open segment meets, in order of t -- the travel field's convention, a diagonal step is allowed
 * whatever lies beside it.  VRC_SIGHT_TOUCH (flags bit 0 set), the supercover: at a tie of the axis set T the walk first visits
 * the voxels reached from the current one by advancing each non-empty proper subset of T, in ascending order of the subset's
 * mask (bit 0 = x, 1 = y, 2 = z), then the voxel with all of T advanced; the visited voxels are exactly those whose closed
 * cube the segment meets.  The walk visits a first, with index 0, and b last; with a == b there is one visited voxel.  The
 * visited SET of b -> a is that of a -> b in both modes.
 *
 * Clear.  A voxel p is clear iff lo <= field(p) <= hi, VRC_DISTANCE_NONE compared as the plain value 0xffffffff
 * (vrc_distance_select's convention).  A thin line of sight on the Euclidean field to the solid: lo = 1, hi = 0xffffffff.  A
 * ball of radius r under vrc_volume_fill_spheres' radius rule: lo = r^2 + 1.  Staying inside the reached medium of a travel
 * field: lo = 0, hi = 0xfffffffe.
 *
 * vrc_sight_segments writes one record per segment (segments: n x 6 int32, a then b).  status = VRC_SIGHT_BLOCKED: `at` is the
 * first visited voxel that is not clear and `before` the voxel visited just before it, `at` itself when `at` is a;
 * VRC_SIGHT_CLEAR: every visited voxel is clear, `at` is b and `before` the voxel visited just before b; VRC_SIGHT_OUTSIDE: an
 * endpoint lies outside the volume, nothing is walked and every other byte is 0.  reserved = 0.  Any vrc_distance snapshot of
 * depth 2..10 is accepted, Euclidean or travel.  mem / stream as in vrc_distance_at: VRC_MEM_HOST stages segments and records
 * in a block of the call's own and is synchronous, VRC_MEM_DEVICE works in place and is asynchronous on `stream`.  A NULL
 * field, NULL buffers with n > 0, lo > hi, unknown flag bits, a bad mem and an n beyond one launch are VRC_ERR_INVALID, refused
 * before any device call; n == 0 is a no-op.  The call keeps no scratch.
 *
 * vrc_sight_field: what an eye sees, as a new vrc_distance snapshot of d's depth on d's device (vrc_travel_connectivity 0).
 * The value at p is |p - eye|^2 when p is in range -- radius == 0, or |p - eye|^2 <= radius^2 -- and every voxel visited by the
 * walk eye -> p is clear, NOT counting p itself; VRC_DISTANCE_NONE otherwise; p == eye always has the value 0.  A solid
 * surface voxel is therefore visible when the air up to it is clear, and an eye inside a wall sees only itself.  Every
 * accessor works on the result: vrc_distance_select(out, 0, r^2, dst, op) is "seen within r", AND-ed with the solid it is the
 * visible blocks; vrc_rigid_clearance on it says which pieces are in view.  stats (may be NULL): visible = the number of
 * finite values, max_d2 = the largest, argmax = the voxel of smallest dense index that holds it, reserved = 0.  Synchronous,
 * on the NULL stream, as the other snapshot creators are; the result owns 4 bytes per voxel, 16 bytes of stats are freed
 * before return.  The cost is ONE WALK PER VOXEL IN RANGE: S^3 walks without a radius.  NULL d or out, an eye outside the
 * volume, lo > hi and unknown flags are VRC_ERR_INVALID.
 *
 * The stride.  On a field made by vrc_volume_distance_field, with hi == 0xffffffff, the walk may STRIDE: such a field is the
 * squared distance to a set, sqrt D is 1-Lipschitz, so the value at a clear voxel bounds how far the segment can be followed
 * without meeting a voxel below lo, and the walk jumps that far and goes on from the voxel the plain walk would be in.  The
 * stride is an optimisation and never part of the rule: the records are byte-identical to the plain walk's (the bound and its
 * proof, and how the kernels are built: DESIGN.md; times: README.md).  Every other snapshot -- a travel field, and a sight field,
 * whose values are no distance to a set although its vrc_travel_connectivity is 0 too --, hi < 0xffffffff and VRC_SIGHT_PLAIN
 * (flags bit 1: so that tests and benchmarks can compare the two on the device) always take the plain walk. */
#define VRC_SIGHT_THIN 0
#define VRC_SIGHT_TOUCH 1
#define VRC_SIGHT_PLAIN 2
#define VRC_SIGHT_CLEAR 0u
#define VRC_SIGHT_BLOCKED 1u
#define VRC_SIGHT_OUTSIDE 2u
typedef struct vrc_sight {      /* 32 bytes */
    uint32_t status;            /* VRC_SIGHT_CLEAR 0, VRC_SIGHT_BLOCKED 1, VRC_SIGHT_OUTSIDE 2 */
    uint32_t at[3];             /* BLOCKED: the first visited voxel that is not clear; CLEAR: b */
    uint32_t before[3];         /* the voxel visited just before `at`; `at` itself when `at` has index 0 */
    uint32_t reserved;          /* 0 */
} vrc_sight;
typedef struct vrc_sight_stats { uint64_t visible; uint32_t max_d2; uint32_t argmax[3]; uint32_t reserved; } vrc_sight_stats;
int vrc_sight_segments(const vrc_distance *d, uint64_t n, const int32_t *segments /* n x 6: a, b */,
                       uint32_t lo, uint32_t hi, int flags, vrc_sight *out, int mem, void *stream);
int vrc_sight_field(const vrc_distance *d, const uint32_t eye[3], uint32_t radius, uint32_t lo, uint32_t hi,
                    int flags, vrc_distance **out, vrc_sight_stats *stats);

/* Deltas: the difference of two volumes as a compact list of changed occupancy words, on the device -- the undo / redo step
 * (an undo stack of clones costs a whole occupancy per step, 16 MiB at 512^3 and 128 MiB at 1024^3, where an edit changes a
 * few hundred words), what carries an edit from the rank that made it to the replicas of the other ranks, and the answer to
 * "what did that edit change".
 *
 * Key, word, bit.  A voxel's key is the one of the components above: with n = S/2 and B = ((x>>1) n + (y>>1)) n + (z>>1),
 * key = 8 B + (z&1) 4 + (y&1) 2 + (x&1).  Its occupancy word is W = key >> 5 and its bit is key & 31.  A volume of depth d
 * has 8^d / 32 words: 2 at 4^3 and 2^25 at 1024^3.
 * Delta.  For two volumes `before` and `after` of one depth on one device, the delta is the list of records
 * { uint32 word, uint32 bits } (8 bytes each) that holds one record for every W with bits = before[W] ^ after[W] != 0, in
 * strictly ascending W.  It is unique and does not depend on scheduling; in numpy, W = flatnonzero(a ^ b), bits = (a ^ b)[W].
 * Apply.  dst[W] ^= bits for every record.  Applied to `before` it gives `after`, applied to `after` it gives `before`: one
 * object serves undo and redo.  Applied to an empty volume it gives the set of changed voxels as a volume, which
 * vrc_volume_copy_region intersects with either state.
 * Stats.  words = the number of records, voxels = the sum of popcount(bits), lo / hi = the bounding box of the changed voxels
 * in setCell coordinates, hi exclusive as in vrc_component; an empty delta has words = voxels = 0 and lo = hi = 0.
 *
 * A vrc_delta is a snapshot as vrc_labels is: it owns its memory (8 bytes per record, nothing for an empty one), is never
 * written after its creator returns, and stays valid when the volumes change or are destroyed.
 *
 * vrc_delta_diff is synchronous (the host reads the record count to allocate exactly 8 * words bytes), on the NULL stream,
 * ordered behind the last asynchronous edit of both volumes; it only reads them and is not recorded as an edit of either.
 * Its scratch (1/256 of an occupancy) belongs to the call and is freed before it returns: vrc_volume_edit_scratch_bytes of both
 * volumes is unchanged.  NULLs (stats may be NULL), before == after, different depths and different devices are
 * VRC_ERR_INVALID, refused before any device call.  The device (csrc/vrc_delta.hip) counts the changed words per workgroup of
 * 256 words -- reducing the voxel count and the box on the way --, scans the counts, and emits; each of the two passes over
 * the fields reads both once, four consecutive words per lane.
 * vrc_delta_create builds a delta from caller records (n x 2 uint32: word, bits) -- another rank's, a saved history's, made by
 * hand.  Synchronous.  With VRC_MEM_DEVICE the records are read in place by a device-to-device copy into the object, so a
 * broadcast can land in the buffer handed to it; they must be complete when the call is made.  One kernel holds the list to
 * the rule -- word strictly ascending, word < 8^depth / 32, bits != 0 -- and reduces the stats.  A list that breaks it is
 * VRC_ERR_INVALID, vrc_last_error names the FIRST offending record index, and no object is returned.  Depth 2..10; n == 0
 * with records == NULL is legal.  stats may be NULL.
 * vrc_delta_get_stats copies the stats kept in the object, vrc_delta_bytes is 8 * count: no device call.
 * vrc_delta_records has the window of vrc_labels_components: the records of [first, first + capacity) that exist go to
 * out[0..] (two uint32 each), nothing beyond them is touched, first >= count writes nothing, capacity == 0 with out == NULL is
 * legal.  VRC_MEM_HOST is staged and synchronous, VRC_MEM_DEVICE is one copy, asynchronous on `stream`.
 * vrc_delta_apply is asynchronous on `stream`, ordered behind dst's last asynchronous edit and recorded as dst's last edit.
 * One lane takes one record; its word is that lane's alone because the words of a list are distinct, so it is a plain load,
 * XOR and store.  The warning of vrc_volume_copy_region holds: do not edit dst on ANOTHER stream before the apply has run.
 * A depth or device mismatch and NULLs are VRC_ERR_INVALID; an empty delta is a no-op that returns VRC_OK.
 * Times: profiles/edit/bench_delta.json (tools/bench_edit.py --delta; 512^3 FastNoise terrain, MI355X, whole calls, device time by
 * events, median of 5, A B A B next to vrc_volume_clone and to a device-to-device copy of one 16 MiB occupancy, 0.008 ms).
 * vrc_delta_diff: 0.072 ms after a radius-8 sphere dig (70 records, 560 bytes), 0.113 ms after dropLoose on the fall benchmark's
 * scene (74877 records, 0.57 MiB), 0.151 ms terrain against empty (300737 records, 2.3 MiB, 14 % of a clone's bytes: the terrain
 * fills less than the half of the words one might expect), next to 0.037 ms for vrc_volume_clone.  vrc_delta_apply: 0.009 ms in
 * all three cases.  So an undo step costs 2 to 4 times a clone's TIME and a 1/30000 to 1/7 of its memory.  The diff is far above
 * the floor of its traffic (two reads of both occupancies, 64 MiB: two of those copies, about 0.02 ms): the call allocates and
 * frees its scratch and its records and reads the count back between scan and emit, and the passes have not been timed apart, so
 * how the rest divides between that host work, the three launches and the kernels is not known. */
typedef struct vrc_delta vrc_delta;      /* a snapshot: the records of a difference, resident on the volumes' device */
typedef struct vrc_delta_stats {         /* 48 bytes */
    uint64_t words;
    uint64_t voxels;
    uint32_t lo[3], hi[3];
    uint32_t reserved[2];                /* 0 */
} vrc_delta_stats;
int vrc_delta_diff(vrc_volume *before, vrc_volume *after, vrc_delta **out, vrc_delta_stats *stats);
int vrc_delta_create(uint32_t depth, int device, uint64_t n, const uint32_t *records /* n x 2 */, int mem,
                     vrc_delta **out, vrc_delta_stats *stats);
int vrc_delta_destroy(vrc_delta *d);
uint64_t vrc_delta_count(const vrc_delta *d);
uint32_t vrc_delta_depth(const vrc_delta *d);
uint64_t vrc_delta_bytes(const vrc_delta *d);      /* 8 * count; pure host bookkeeping */
int vrc_delta_get_stats(const vrc_delta *d, vrc_delta_stats *out);   /* host copy kept in the object, no device call */
int vrc_delta_records(const vrc_delta *d, uint64_t first, uint64_t capacity, uint32_t *out, int mem, void *stream);
int vrc_delta_apply(const vrc_delta *d, vrc_volume *dst, void *stream);

/* Sparse tile stream: a volume as a byte stream that is small where the world is solid rock or air, packed and unpacked on
 * the device -- the saved game, the level file, the first sync of a replica, the base that deltas apply to.  (vrc_volume_download
 * is one byte per voxel, 128 MiB at 512^3; there was no direct way back in.)
 *
 * Format, version 1.  Little-endian; every section starts on a multiple of 4 bytes.  With S = 1 << depth (depth 2..10):
 *   n = S/2 bricks per axis, E = min(8, n) the tile edge in bricks, T = n/E tiles per axis, NT = T^3 tiles, K = E^3 bricks per
 *   tile (8, 64 or 512), MW = max(1, K/32) words per mask (1, 2 or 16).
 * Brick: the 2 x 2 x 2 voxels with brick coordinates (x>>1, y>>1, z>>1); its byte has bit (z&1) 4 + (y&1) 2 + (x&1), the
 * occupancy's own bits (key & 7 above).  Tile (tx, ty, tz) holds the bricks (E tx + i, E ty + j, E tz + k); its index is
 * t = (tx T + ty) T + tz and a brick's local index q = (i E + j) E + k.  Tile class: 0 = every brick byte 0, 1 = every brick
 * byte 0xff, 2 = mixed; 3 is illegal.  Mixed tiles are numbered by rank r in ascending t.  A partial brick is a brick of a
 * mixed tile whose byte is neither 0 nor 0xff.
 *   Header, 64 bytes = 16 uint32: 0 magic 0x50435256 (the bytes V R C P), 1 version 1, 2 depth, 3 NT, 4 M = mixed tiles,
 *     5 P = partial bricks, 6..7 the stream's length in bytes (uint64, low word first), 8..9 solid voxels (uint64),
 *     10 class-1 (full) tiles, 11..15 zero.
 *   A, class map: ceil(NT/16) uint32; the class of tile t in bits 2(t%16), 2(t%16)+1 of word t/16, unused bits 0.
 *   B, counts: M uint32; entry r = the partial bricks of mixed tile r.
 *   C, masks: M x 2 MW uint32; per mixed tile first `some` (bit q%32 of word q/32 set iff the brick byte is not 0), then
 *     `full` (set iff it is 0xff); bits at q >= K are 0 (depth 2 alone has them).
 *   D, partial bytes: P bytes, tiles in ascending rank and within a tile in ascending q; then 0..3 zero bytes.
 * Length = 64 + 4 ceil(NT/16) + 4 M + 8 MW M + 4 ceil(P/4); vrc_pack_bound(depth) is this with M = NT and P = n^3 (0 for a
 * depth outside 2..10): 712 bytes at 16^3 and about 1.26 x the occupancy from 32^3 up (20.1 MiB at 512^3).  A volume has
 * exactly one stream: equal occupancies give equal bytes, and pack(unpack(s)) == s for every s that unpack accepts.
 *
 * Canonical rules.  A stream is accepted only if all hold; vrc_last_error names the first that does not, in this order, as
 * "rule <name>", for the rules marked (tile) / (byte) followed by " at tile <t>" / " at byte <offset into the stream>" with the
 * LEAST offender.  From the 64 header bytes, on the host, before any kernel reads a section:
 *   header-short     at least 64 bytes;
 *   magic-version    magic and version match;
 *   depth            the depth is 2..10 and, for vrc_unpack_volume, the volume's;
 *   tiles            the NT word is right;
 *   reserved         words 11..15 are 0;
 *   length-argument  the length word equals the `bytes` argument;
 *   length-formula   the length word equals the formula with the header's M and P;
 *   count-limits     M <= NT, P <= K M, full + M <= NT.
 * On the device:
 *   class-map (tile)      no class 3, no unused bit set (reported as the tile index the field would have);
 *   mixed-count           the class-2 tiles are M;
 *   full-count            the class-1 tiles are header word 10;
 *   full-in-some (tile)   full is a subset of some;
 *   mask-range (tile)     no mask bit at q >= K;
 *   some-empty (tile)     some != 0;
 *   full-whole (tile)     full does not have all K bits;
 *   partial-count (tile)  popcount(some & ~full) equals the tile's B entry;
 *   partial-sum           the sum of B equals P;
 *   partial-byte (byte)   no D byte is 0x00 or 0xff;
 *   padding (byte)        the padding is zero;
 *   solid-count           the solid voxels counted from the stream equal header words 8, 9.
 * The mask rules are evaluated for the mixed tiles of rank < M.  A refused stream is VRC_ERR_INVALID and the volume keeps its
 * occupancy bit for bit: no kernel reads outside [data, data + bytes) or writes the occupancy before every check has passed,
 * and an offset into D stays below P whatever B claims.
 *
 * vrc_pack_header is pure host: the header rules (any depth in 2..10) over the first 64 bytes, and the header's fields.
 * vrc_pack_volume and vrc_unpack_volume are synchronous like vrc_volume_commit and vrc_volume_clone: on the NULL stream, behind
 * the volume's last asynchronous edit.  `mem` says where out / data live; info is always host memory.  Host memory is staged
 * through a device block of the stream's length that belongs to the call and is freed before it returns.
 * vrc_pack_volume: out == NULL with capacity == 0 runs the count and scan passes only and fills info.  capacity < info->bytes
 * is VRC_ERR_INVALID with info filled and nothing written; otherwise exactly info->bytes bytes are written and nothing beyond
 * them is touched.  A device `out` must be 4-byte aligned; a misaligned one is refused and not written.
 * vrc_unpack_volume replaces the whole occupancy.  With device `data` the 64 header bytes are copied to the host first; device
 * `data` must be 4-byte aligned and complete when the call is made.
 * NULLs, a bad `mem`, out == NULL with capacity > 0 and a misaligned device buffer are VRC_ERR_INVALID before any device call.
 * Scratch: the per-tile slots and the totals, 8 (NT + 1) + 64 bytes (2 MiB at 1024^3, 256 KiB at 512^3), one block of the
 * volume, allocated by the first of the two calls, never grown, counted by vrc_volume_edit_scratch_bytes from then on.
 * The device (csrc/vrc_pack.hip): pack is count -> scan -> emit with one 64-lane wave per tile, a lane per row of 8 brick bytes,
 * no workgroup waiting for another; unpack is class count and rank scan, mask checks and offset scan, the D check, and only then
 * the write, a wave per tile.  The two calls are named vrc_pack_volume / vrc_unpack_volume, not vrc_volume_*.
 * Times: profiles/edit/bench_pack.json (tools/bench_edit.py --pack; 512^3 on the MI355X, whole calls, device time by events,
 * median of 5, in one run next to vrc_volume_clone, 0.05 to 0.06 ms, and vrc_volume_download, 2.7 to 2.9 ms for 128 MiB).
 * FastNoise terrain: 517316 bytes (M = 2849 of 32768 tiles, P = 132990; 3.1 % of the 16 MiB occupancy), size-only call 0.150 ms,
 * pack to device memory 0.166 ms, unpack from device memory 0.175 ms.  A 0.5-density random field, the format's worst case:
 * 20979956 bytes (M = 32768, P = 16646321; 1.25 x the occupancy: LARGER than what it stands for), size-only 0.484 ms, pack
 * 0.542 ms, unpack 0.246 ms.  A pack or unpack costs 3 to 10 clones in time.  The size-only call is nearly the whole pack, and
 * the count pass is three times slower on the random field over the same 16 MiB: every one of its 32768 waves adds to the one
 * solid counter there.  The passes have not been timed apart. */
typedef struct vrc_pack_info {           /* 40 bytes */
    uint32_t depth, tiles, mixed_tiles, full_tiles, partial_bricks, reserved;
    uint64_t bytes, solid;
} vrc_pack_info;
uint64_t vrc_pack_bound(uint32_t depth);                                   /* pure host; 0 for a bad depth */
int vrc_pack_header(const void *data, uint64_t bytes, vrc_pack_info *out); /* pure host */
int vrc_pack_volume(vrc_volume *v, void *out, uint64_t capacity, vrc_pack_info *info, int mem);
int vrc_unpack_volume(vrc_volume *v, const void *data, uint64_t bytes, int mem);

/* Cells: the local question -- how many of a voxel's neighbours are solid -- as one step of a neighbour-count automaton,
 * and a voxel set from a seed.  Clean-up (specks a brush or a fracture leaves, pin-holes), rounding by a majority vote,
 * caves from a random fill and a few rounds of a rule, 3-D Life: all are one stencil.  (vrc_distance_select's grow / shrink is
 * another operator: it moves the whole surface by r and costs a distance transform.)
 *
 * vrc_cells_step.  For every voxel p of src, c(p) is the number of solid voxels among its `neighbours` neighbours: the six
 * that share a face (VRC_CELLS_FACES), or the 26 that share a face, an edge or a corner (VRC_CELLS_ALL).  A neighbour outside
 * the volume counts as empty when outside == 0 and as solid when outside == 1.  Then
 *     dst(p) = (survive_mask >> c(p)) & 1  if src(p) is solid,  (birth_mask >> c(p)) & 1  if it is empty.
 * dst is written whole, whatever it held; src is only read.  The result is unique and does not depend on scheduling.
 * `changed` may be NULL; otherwise it receives the number of voxels with dst(p) != src(p), and `mem` says where it lives:
 * VRC_MEM_HOST makes the call synchronous, VRC_MEM_DEVICE is one device uint64_t, zeroed and written in stream order -- a
 * caller that iterates to a fixed point reads it once every few steps.  The ordering is vrc_volume_copy_region's: the call is
 * asynchronous on `stream`, runs behind the last asynchronous edits of both volumes and is recorded as dst's last edit.
 * VRC_ERR_INVALID with the function's name, before any device call: NULL volumes, dst == src, different depths or devices,
 * neighbours not 6 or 26, a mask bit above bit `neighbours` (no count reaches it: a typo, not a rule), outside not 0 or 1,
 * and a bad `mem` when changed is given.  No scratch: vrc_volume_edit_scratch_bytes of both volumes is unchanged.
 * The device (csrc/vrc_cells.hip): one lane owns one destination word (2 x 2 x 8 voxels) and writes it once.  It counts all 32
 * voxels at a time on bit-planes: the nine brick rows around the word are shifted to the word's bit positions with the
 * flood's shifts, a full adder along x gives 2 planes, along y 4, along z 5 -- the count of the 27 cells with the centre,
 * which is folded into the rule (a solid centre reads survive_mask << 1) -- and the rule is a select tree over the planes with
 * the masks' bits as leaves.  The six-neighbour count is a direct sum of six planes.
 *
 * vrc_cells_fill_random.  With L(u), the 32-bit finaliser
 *     u ^= u >> 16;  u *= 0x7feb352d;  u ^= u >> 15;  u *= 0x846ca68b;  u ^= u >> 16      (all mod 2^32),
 * h(x, y, z) = L(L(L(L(seed) ^ x) ^ y) ^ z) and R(p) = (h(p) < threshold), compared in 64 bits: threshold 0 selects nothing,
 * 2^32 everything, a density d is threshold = round(d 2^32); above 2^32 is VRC_ERR_INVALID.  Inside the box lo_hi (6 uint32:
 * lo inclusive, hi exclusive, clipped to the volume; NULL = the whole volume) v becomes R (VRC_COPY_REPLACE), v | R
 * (VRC_COPY_OR) or v & ~R (VRC_COPY_ANDNOT); nothing outside the box is touched, and an empty or inverted box is a legal
 * no-op.  The hash takes coordinates, not keys, so the field is the same at every depth and in every box.  The nesting
 * order is deliberate: an occupancy word is 2 x 2 x 8 voxels, so it needs L(seed) once (the host computes it), 2 values for
 * its x, 4 for its (x, y) and 32 for its z -- 38 evaluations of L for 32 voxels.  Asynchronous on `stream`, behind v's last
 * asynchronous edit, recorded as v's last edit.  A NULL volume, a threshold above 2^32 and an unknown op are
 * VRC_ERR_INVALID before any device call.
 * Times: profiles/edit/bench_cells.json (tools/bench_edit.py --cells; 512^3 on the MI355X, device time by events around 20 calls in
 * a row, median of 5, A B A B next to a whole-volume vrc_volume_copy_region, 0.060 ms, and vrc_volume_clone, 0.036 ms), alike on
 * the FastNoise terrain and on a 0.5 random fill: a step with 6 neighbours 0.031 ms, with 26 neighbours 0.066 ms, the fill of the
 * whole volume 0.060 ms.  With `changed` in device memory a step costs 0.038 / 0.076 ms on the terrain, where few workgroups
 * change anything, and 0.21 ms on the random fill, where every one of 16384 workgroups adds to the same counter: ask for the
 * count once every few steps. */
#define VRC_CELLS_FACES 6      /* the six face neighbours  */
#define VRC_CELLS_ALL   26     /* faces, edges and corners */
int vrc_cells_step(vrc_volume *dst, vrc_volume *src, int neighbours, uint32_t birth_mask, uint32_t survive_mask, int outside,
                   uint64_t *changed, int mem, void *stream);
int vrc_cells_fill_random(vrc_volume *v, uint32_t seed, uint64_t threshold, const uint32_t *lo_hi /* 6, NULL = whole volume */,
                          int op, void *stream);

/* Columns: the volume looked at, and written, along an axis -- a height map out of a volume, a volume out of height maps, and
 * the voxels a parallel light reaches.  `axis` is 0, 1, 2 for x, y, z and direction = 2 * axis + side as for vrc_fall_drops:
 * side 0 travels towards smaller coordinates (it enters at the high face), side 1 towards larger ones.  A COLUMN is the S
 * voxels that differ only in the axis coordinate.  The other two axes in x < y < z order are (u, v): a map of the whole face
 * has S x S entries, column (u, v) at u * S + v -- for axis 1 this is height[x * S + z] of vrc_scene_build_terrain.  `rect` is
 * 4 uint32 (u_lo, v_lo, u_hi, v_hi), lo inclusive, hi exclusive, NULL = the whole face; it must be non-empty and lie inside
 * [0, S]^2 and is NOT clipped (a clipped rect would change the stride of the caller's arrays): the maps of a rect are dense
 * (u_hi - u_lo) x (v_hi - v_lo) arrays, column (u, v) at (u - u_lo) * (v_hi - v_lo) + (v - v_lo).
 *
 * vrc_columns_profile.  Per column of the rect, travelling along the direction from the entry face: `first` is the axis
 * coordinate of the first solid voxel met, `last` that of the last one, `count` the number of solid voxels and `runs` the
 * number of maximal runs of consecutive solid voxels; an empty column is (VRC_COLUMN_NONE, VRC_COLUMN_NONE, 0, 0).  A column
 * with runs == 1 whose run touches the exit face is a height-field column: no overhang, no cave.  `first` is the height map,
 * `count` the thickness (X-ray) image, count != 0 the silhouette.  The call reads the occupancy: it runs on `stream` behind
 * the volume's last asynchronous edit and is not an edit; `mem` says where out lives, and VRC_MEM_HOST makes the call
 * synchronous.  Every record of the rect is written once and nothing else is.
 *
 * vrc_columns_fill.  Per column of the rect the span is [lo, hi) along `axis`: lo is the column's entry of lo_map, or lo_const
 * when lo_map is NULL, and hi likewise; both are int32 and clamped to [0, S], and lo >= hi is an empty span.  Under
 * VRC_COPY_REPLACE the column becomes exactly its span (the rest of the column is cleared), under VRC_COPY_OR the span is set,
 * under VRC_COPY_ANDNOT it is cleared; nothing outside the rect's columns is touched.  Both maps NULL is a box fill.  With
 * axis 1, lo_const = S/2 + 1, hi = S/2 + clamp(height, 16, S) and REPLACE on an empty volume this is the terrain of
 * vrc_scene_build_terrain, as a volume one can dig in.  `mem` says where the maps live.  The call is an edit on `stream`,
 * behind the volume's last asynchronous edit and recorded as its last edit; VRC_MEM_HOST makes it synchronous.
 *
 * vrc_columns_select.  For a voxel p of src, P(p) is the number of solid voxels met before p (p not counted) when travelling
 * along the direction through p's column.  K = { p : lo <= P(p) < hi, and p is solid (of = VRC_COLUMNS_SOLID), empty
 * (VRC_COLUMNS_EMPTY) or either (both bits) }, and dst becomes K (VRC_COPY_REPLACE), dst | K or dst & ~K over the whole volume.
 * (0, 1, SOLID) is the lit surface, one voxel per non-empty column, at the profile's `first`; (0, 1, EMPTY) the open sky;
 * (0, k, SOLID) the top k solid voxels of every column; (1, S + 1, EMPTY) everything under a roof, overhangs and caves alike.
 * No count reaches S, so a bound above S + 1 means S + 1; lo > hi as given is refused, lo == hi selects nothing.  The ordering
 * is vrc_cells_step's: asynchronous on `stream`, behind the last asynchronous edits of both volumes, recorded as dst's last
 * edit; src is only read.  dst == src is refused as vrc_cells_step refuses it: clone first.
 *
 * VRC_ERR_INVALID as "<function>: <reason>", before any device call: NULL volumes, a NULL out, a direction outside 0..5, an
 * axis outside 0..2, a rect that is empty or reaches beyond S, an unknown op, `of` or `mem`, lo > hi, dst == src, volumes of
 * different depths or devices.  Host-memory lists (out, the maps) are staged in a block of the call's own, freed before it
 * returns: vrc_volume_edit_scratch_bytes is unchanged by all three calls.
 * The device (csrc/vrc_columns.hip): a word is 2 x 2 x 8 voxels, so 16 columns cross it along x or y, two levels each, and 4
 * along z, eight levels each.  Profile and select give the columns that cross one word to ONE lane, which walks the words
 * they cross from face to face -- a stride of a brick plane along x, of a brick row along y, consecutive words along z; along
 * x and y adjacent lanes take adjacent words -- and carries the columns' state as bit masks and bit-planes over a level's
 * column positions: seen / previous masks, first and last as planes of the level's coordinate, count and runs by a ripple add
 * of one bit; select keeps P - lo and P - hi in two's complement and reads the band off the two sign planes.  No atomics, no
 * cross-lane step, every word read once, every record and every dst word written once.  Fill is one lane per destination
 * word of the box  rect x the whole axis, which reads the spans of the word's 4 (z) or 16 (x, y) columns and stores the word
 * once under the box's mask (4^3: two brick rows share a word and its halves take atomics).
 * Times: profiles/edit/bench_columns.json (tools/bench_edit.py --columns; 512^3 on the MI355X, every list in device memory, device
 * time by events around 20 calls in a row, median of 5, A B A B next to the yardstick named), alike on the FastNoise terrain and
 * on a 0.5 random fill.  The profile of the whole face, 4 MiB of records: 0.078 ms along x, 0.080 ms along y, 0.069 ms along z,
 * next to vrc_volume_clone, 0.037 ms (2.1, 2.2 and 1.9 clones), and vrc_volume_solid_count, 0.025 ms on the terrain (3.1, 3.3, 2.7
 * counts) and 0.067 ms on the random fill (1.1, 1.2, 1.1).  The fill along y from the 512^2 FastNoise heights (the terrain,
 * REPLACE): 0.113 ms next to 0.023 ms for a whole-volume vrc_volume_fill_boxes, 4.9 of them: each of the 4 Mi lanes reads the
 * spans of its word's 16 columns, so the 1 MiB map goes through the caches 256 times -- what the code suggests, not measured
 * apart.  The select (0, 1, SOLID): 0.077 ms along x and y, 0.066 ms along z, next to 0.031 to 0.032 ms for a 6-neighbour
 * vrc_cells_step (2.4, 2.4 and 2.1 steps).  No axis stands out; the walks are one lane per bundle, 16384 lanes along x and y
 * and 65536 along z at this size, each with 512 levels of bit-plane arithmetic behind its loads. */
typedef struct vrc_column { uint32_t first, last, count, runs; } vrc_column;   /* 16 bytes */
#define VRC_COLUMN_NONE   0xffffffffu
#define VRC_COLUMNS_SOLID 1
#define VRC_COLUMNS_EMPTY 2      /* 3 = both */
int vrc_columns_profile(vrc_volume *v, int direction, const uint32_t *rect /* 4, NULL = whole face */, vrc_column *out, int mem,
                        void *stream);
int vrc_columns_fill(vrc_volume *v, int axis, const uint32_t *rect /* 4, NULL = whole face */, const int32_t *lo_map, int32_t lo_const,
                     const int32_t *hi_map, int32_t hi_const, int op, int mem, void *stream);
int vrc_columns_select(vrc_volume *dst, vrc_volume *src, int direction, uint32_t lo, uint32_t hi, int of, int op, void *stream);

/* Levels: voxels between volumes of two depths -- the density grid of a volume, the coarse volume selected by it, and a coarse
 * volume blown up again.  k >= 1 is a level difference.  A CELL of level k is the cube of 2^k voxels per axis whose low corner
 * is a multiple of 2^k on every axis: cell (X, Y, Z) of a volume of size S holds the voxels p with p >> k == (X, Y, Z), there
 * are S_c = S >> k cells per axis, and count(X, Y, Z) is the number of solid voxels in the cell, 0 .. 8^k.  The calls that cross
 * depths otherwise (vrc_volume_stamp_affine, the posed pieces) point-sample: a stamp with scale 1/2 keeps one voxel of eight.
 *
 * vrc_levels_counts.  k is in 1 .. depth(src).  counts has S_c^3 entries in the dense order counts[(X * S_c + Y) * S_c + Z], the
 * order of vrc_volume_download's solid[(x * S + y) * S + z]; every entry is written exactly once with the exact count (the
 * largest, 8^10 = 2^30, fits), and k = depth gives one entry, the volume's solid count.  `mem` says where counts lives:
 * VRC_MEM_HOST is staged in a block of the call's own and makes the call synchronous, VRC_MEM_DEVICE works in place and is
 * asynchronous on `stream`.  Either way the call runs behind src's last asynchronous edit and is not an edit itself.  Two calls
 * give identical bytes.
 *
 * vrc_levels_reduce.  depth(dst) < depth(src), and k is their difference: voxel P of dst is cell P of src.  With
 * K = { P in dst : lo <= count(P) < hi }, dst becomes K (VRC_COPY_REPLACE), dst | K (VRC_COPY_OR) or dst & ~K (VRC_COPY_ANDNOT)
 * over the whole of dst, as vrc_columns_select does it.  "Any voxel solid", the conservative proxy, is (1, 8^k + 1); "all solid",
 * the interior, is (8^k, 8^k + 1); "at least half", which keeps the volume, is (8^k / 2, 8^k + 1); the empty cells are (0, 1).
 * lo >= hi is a legal empty K, and an hi above 8^k + 1 means 8^k + 1.  Thresholds do not compose: reduce every level from the
 * finest volume, not from the level before, unless the rule is "any" or "all".
 *
 * vrc_levels_expand.  depth(dst) > depth(src), k their difference.  With E = { p in dst : src(p >> k) solid }, dst becomes E,
 * dst | E or dst & ~E over the whole of dst.  It is vrc_volume_stamp_affine with m = diag(65536 >> k), t = 0, bit for bit.
 *
 * Reduce and expand take two different volumes on one device, are asynchronous on `stream`, run behind the last asynchronous
 * edits of both volumes and are recorded as dst's last edit; src is only read.  As for vrc_volume_copy_region, an edit of
 * either volume that is still in flight on ANOTHER stream and was issued after the call is not ordered against it.
 * VRC_ERR_INVALID as "<function>: <reason>", before any device call: a NULL volume, NULL counts, dst == src, volumes on
 * different devices, k == 0 or k > depth, depth(dst) >= depth(src) for reduce and depth(dst) <= depth(src) for expand, an
 * unknown op or mem.  vrc_volume_edit_scratch_bytes is unchanged by all three calls.
 * The device (csrc/vrc_levels.hip, the switches: csrc/vrc_levels.h): a brick byte is a cell of level 1 and its count a
 * popcount.  counts: k = 1 a lane per source word, four counts each; k = 2, 3 a lane per cell, 4 loads of two bytes or 16 of a
 * word; k >= 4 a workgroup per 2048 words of a cell, summed over the group, and from k = 6, where a cell has several
 * workgroups, added with 32-bit vector atomics onto counts zeroed on the stream -- integer sums, so the bytes are the same
 * every time.  reduce: k = 1 a lane per dst word, which is four rows of eight contiguous source bytes; else a lane per dst
 * voxel that counts its cell (k = 2, 3) or reads the count from a grow-only block of dst's, at most 1 MiB (k >= 4: dst has depth
 * 6 at the most), the word being one ballot of its 32 lanes.  expand: a lane per dst word, at most four source bytes read.
 * Every dst word has one owner and is stored whole, 4^3 included.
 * Times: profiles/edit/levels_timing.json (tools/bench_levels.py; 512^3 on the MI355X, the counts in device memory, device time
 * by events around 10 calls in a row, median of 5, the yardsticks in the same rounds; the 16 MiB source stays in the last-level
 * cache from call to call, for the yardsticks alike), FastNoise terrain / 0.5 random field.  counts: k = 1 0.012 / 0.014 ms (64 MiB
 * of counts written), k = 3 0.005 / 0.005 ms, k = 5 0.021 / 0.021 ms, k = 9 0.010 / 0.028 ms, next to vrc_volume_clone of the source,
 * 0.052 / 0.049 ms -- a weak yardstick, it allocates and synchronises, so the expectation "k = 1 costs a clone" is not what was
 * measured: 0.24 / 0.27 of one -- and vrc_volume_solid_count, 0.026 / 0.068 ms, of which k = 9, the same number, is 0.38 / 0.42.
 * k = 5 is the slowest form, four times k = 3: a cell's rows reach its workgroup in pieces of 16 bytes; k = 9 on the random
 * field adds 2048 workgroup sums onto one word, where the terrain's empty workgroups add nothing -- what the code suggests,
 * not measured apart.  reduce "any": to 256^3 0.008 ms, to 64^3 0.007 ms, to 4^3 (counts into the block,
 * then the select) 0.015 / 0.023 ms.  expand 256^3 to 512^3: 0.013 / 0.014 ms next to 0.114 / 0.115 ms for
 * vrc_volume_stamp_affine with m = diag(32768), 8.5 and 8.4 times faster.  No form is slower than its yardstick. */
int vrc_levels_counts(vrc_volume *src, uint32_t k, uint32_t *counts, int mem, void *stream);
int vrc_levels_reduce(vrc_volume *dst, vrc_volume *src, uint32_t lo, uint32_t hi, int op, void *stream);
int vrc_levels_expand(vrc_volume *dst, vrc_volume *src, int op, void *stream);

/* Morphology with a structuring element of the caller's choice: the Minkowski sum and difference of a voxel set with a box, a
 * line, a cross, a ball or the voxels of a piece.  (vrc_distance_select's grow / shrink knows the ball alone and builds a field of
 * 4 bytes a voxel for it; vrc_cells_step reaches one voxel.)  "Grow by 3 x 5 x 3", "smear 6 voxels along +x", "where does THIS
 * shape fit" -- erode the empty voxels by the shape, and vrc_travel_field through the result is the shortest path of a shaped
 * agent -- and pattern search (hit-or-miss) are this one call.
 *
 * vrc_morph_apply.  The rule:
 *   The set A.  Inside the volume, A holds the voxels of src that are solid (of == VRC_MORPH_SOLID) or empty (VRC_MORPH_EMPTY).
 *     Beyond the faces, every lattice point belongs to A iff outside != 0.
 *   The element E.  E = { offsets[i] - origin : 0 <= i < n } as a set; duplicates are legal.  Subtracting `origin` lets a
 *     uint32 x y z list from vrc_voxels_extract (values below 2^31) be passed unchanged, with `origin` as the pivot: a piece
 *     becomes an element without a host copy.
 *   DILATE.  K = { p in the volume : some e in E has p - e in A }, that is A (+) E.
 *   ERODE.   K = { p in the volume : every e in E has p + e in A }, that is A (-) E.
 *   n == 0.  DILATE gives K empty, ERODE gives K the whole volume: the formulas taken literally, and legal.
 *   dst becomes K (VRC_COPY_REPLACE), dst | K (VRC_COPY_OR) or dst & ~K (VRC_COPY_ANDNOT) over the whole of dst, as
 *     vrc_columns_select does it.  src is only read.  The result is unique and does not depend on scheduling.
 *   Duality.  ERODE(of, E, outside) is the complement of DILATE(the other `of`, -E, !outside).
 * Minkowski sums compose: the dilation by a box a x b x c is three dilations by lines in a row, a + b + c offsets for a b c.
 * The call is vrc_cells_step's kind: two different volumes of one depth on one device, asynchronous on `stream`, behind the last
 * asynchronous edits of both volumes, recorded as dst's last edit.  `mem` says where `offsets` (n x 3 int32) lives:
 * VRC_MEM_HOST stages the list in a block of the call's own and makes the call synchronous, VRC_MEM_DEVICE reads it in place.
 * `origin` is three host ints (NULL = 0 0 0), read before the call returns.  vrc_volume_edit_scratch_bytes of both volumes is
 * unchanged: the prepared element lives in a block of dst's own, 13312 bytes, allocated by the first call and fixed in size.
 * VRC_ERR_INVALID as "vrc_morph_apply: <reason>", before any device call: NULL volumes, dst == src, different depths or devices,
 * an unknown what, of, op or mem, outside not 0 or 1, n above VRC_MORPH_MAX_OFFSETS, NULL offsets with n != 0 and, in host
 * memory, an offset with a component beyond +-VRC_MORPH_REACH after the origin is subtracted (in 64 bits; the text names the
 * least such index).  In device memory the host cannot look: such an offset is DROPPED, which is vrc_volume_set_voxels's rule
 * for coordinates outside.
 * The device (csrc/vrc_morph.hip): a lane per offset ORs bit ez + 16 into the 64-bit z mask of column (ex, ey) of a 33 x 33 table
 * (8712 bytes) -- duplicates fall together, what is out of reach falls out -- and one workgroup lists the non-empty columns and
 * the element's box.  ERODE and `of` EMPTY are the same loop by the duality: complement on load, the list read negated,
 * complement on store.  A workgroup owns 32 x 32 voxel columns and 32 voxels of z.  It brings the source in with the halo of the
 * element's own box as PILLARS in LDS, per voxel column the 64 z bits from 16 below the tile, where a step along x or y is an
 * index and a step along z a shift; a lane owns a brick column of the tile, four words along z, and per listed column ORs one
 * shifted copy of its four pillars per set bit of the mask.  The cost follows the element's non-empty columns and the bits of
 * their masks, not n and not the 33^3 cube.  Every dst word has one owner and is stored whole and once, without atomics, 4^3
 * included.
 * Times: profiles/edit/morph_timing.json (tools/bench_morph.py; 512^3 on the MI355X, the list in device memory, DILATE into a second volume, device
 * time by events around 10 calls in a row, median of 5, A B A B with the yardstick in the same rounds and giving the same bits), FastNoise
 * terrain / 0.5 random field.  The 3 x 3 x 3 cube 0.066 / 0.070 ms next to 0.069 / 0.071 ms for a 26-neighbour vrc_cells_step, 0.96 / 0.99 of it.
 * The cross 0.058 / 0.059 ms next to 0.031 / 0.032 ms for the 6-neighbour step: 1.9 times SLOWER, the staging of the pillars is the floor
 * of every call.  element_ball(r): r = 2 0.069 ms, r = 4 0.161 / 0.168 ms, r = 8 0.783 / 0.811 ms, next to 2.9 / 5.1 ms for
 * vrc_volume_distance_field + vrc_distance_select whatever r, 42 / 74, 18 / 31 and 3.7 / 6.3 times faster, holding 13312 bytes where the field
 * holds 512 MiB.  The cost follows the mask bits (33, 257, 2109 offsets: x 4.9 from r = 4 to r = 8), so no crossover was measured up to
 * r = 8; at that growth the ball of r = 16 would cost 4 to 6 ms, about the field's time: the crossover lies near the reach, not
 * measured.  The 9 x 9 x 9 box as one call 0.312 / 0.321 ms next to 0.154 / 0.155 ms for three line calls, 2.0 times SLOWER: compose boxes from
 * lines.  The 33-voxel line 0.090 / 0.092 ms along x, 0.088 / 0.089 ms along y, 0.056 ms along z, where it is one column of 33 bits. */
#define VRC_MORPH_DILATE 0
#define VRC_MORPH_ERODE  1
#define VRC_MORPH_SOLID  1      /* the set A is src's solid voxels */
#define VRC_MORPH_EMPTY  2      /* ... src's empty voxels          */
#define VRC_MORPH_REACH  16     /* |component of an offset| <= 16  */
#define VRC_MORPH_MAX_OFFSETS (1u << 20)
int vrc_morph_apply(vrc_volume *dst, vrc_volume *src, int what, int of, uint64_t n, const int32_t *offsets /* n x 3 */,
                    const int32_t *origin /* 3, NULL = 0 */, int outside, int op, int mem, void *stream);

/* ---- dense grid: Grid3D<X,Y,Z> (grid_3d.hpp:10-138) ------------------- */

/* cells[(x*Y + y)*Z + z] = Cell::Type (0 = Empty). */
int vrc_grid_create(const uint8_t *cells, int32_t X, int32_t Y, int32_t Z, int device, vrc_grid **out);
int vrc_grid_destroy(vrc_grid *g);
/* Grid3D::castRay(position, direction) (grid_3d.hpp:36-132), voxel units.  The start cell is the origin truncated towards
 * zero (:58-60: an origin in (-1, 0) starts in cell 0).  An origin coordinate that is NaN or outside [-2^31, 2^31) has no
 * cell: the ray is a miss with an all-zero record, complexity included, as in the reference as it ships (x86-64 converts
 * such a value to INT_MIN, and the loop at :70 never runs).  So is every ray whose start cell lies outside the grid.
 * Non-finite and zero direction components are valid input and give what the reference's arithmetic gives; the sign and
 * payload of a NaN in a float field are the hardware's. */
int vrc_grid_cast_rays(const vrc_grid *g, uint64_t n, const float *org_xyz, const float *dir_xyz,
                       vrc_hit *out, int mem, void *stream);

/* ---- per-frame operator: RayCaster (raycaster.hpp:43-283) ------------- */

/* Camera (camera_controller.hpp:16-61).  The Camera class itself stays on the
 * host; these are the values Camera::getRay reads. */
typedef struct vrc_camera {
    float position[3];      /* world voxel units */
    float rot[9];           /* glm::mat3 rot_mat, columns m[0], m[1], m[2] */
    float fov;
    float aperture;
    float focal_length;
} vrc_camera;

typedef struct vrc_frame_params {
    float light_position[3];  /* RayCaster::setLightPosition (raycaster.hpp:62), SVO space */
    uint32_t use_gi;          /* raycaster.hpp:274 */
    uint32_t use_samples;     /* raycaster.hpp:275 */
    uint32_t shadow_samples;  /* 0 = reference default: use_samples ? 4 : 1 (raycaster.hpp:147) */
    uint32_t gi_bounces;      /* 0/1 = reference (one indirect bounce); 2 = extension */
    int32_t checker_parity;   /* -1 = every pixel; 0/1 = checker_board_offset (main.cpp:137,143) */
    uint32_t spp;             /* renderRay-equivalents per pixel in this call (1 .. 65536) */
    uint32_t seed;            /* counter-based RNG key ... */
    uint32_t frame_index;     /* ... sample s of this call uses frame_index + s */
    uint32_t row_block;       /* multi-GPU: rows per shard block (0 = whole frame) */
    uint32_t shard_index;     /* this renderer renders row blocks b with b % shard_count == shard_index */
    uint32_t shard_count;
} vrc_frame_params;

typedef struct vrc_frame_stats {
    uint64_t rays;            /* LSVO::castRay-equivalent traversals executed */
    uint64_t sum_complexity;  /* sum of HitPoint::complexity over them (8 B each = algorithmic bytes) */
    uint64_t primary_hits;
    uint64_t pixels;          /* pixel-samples shaded */
    uint64_t iterations_not_executed;  /* the part of sum_complexity the frame kernels counted without executing: a ray next to
                                        * the previous hit (or the camera) starts below the root, at the end of the descends
                                        * that lsvo.hpp:72-111 would make from the root (same walk, same count) */
} vrc_frame_stats;

/* Streams for hosts that do not link the HIP runtime themselves: every `void *stream` argument of
 * this header is a hipStream_t (NULL = the default stream).  A host that keeps frames in flight
 *  needs one stream per frame in flight. */
int vrc_stream_create(int device, void **stream);
int vrc_stream_destroy(int device, void *stream);
int vrc_stream_synchronize(int device, void *stream);   /* blocks the calling thread until the stream's work is done */

/* RayCaster(svo, render_size) (raycaster.hpp:48-60): framebuffer cleared to
 * opaque black (sf::Image::create), accumulators zero.  The scene must outlive
 * every vrc_render_frame call on the renderer (as `const LSVO<9>& svo` must
 * outlive the RayCaster, raycaster.hpp:265); the other renderer calls and
 * vrc_renderer_destroy do not touch it.  The renderer takes a snapshot of the
 * process-wide scheduling defaults (vrc_set_*) at creation. */
int vrc_renderer_create(const vrc_scene *s, uint32_t width, uint32_t height, vrc_renderer **out);
int vrc_renderer_destroy(vrc_renderer *r);
/* Points the renderer at another scene of the same depth on the same device (e.g. the one vrc_volume_commit just
 * built), between its frames: frames already enqueued keep the scene they were enqueued with, so the old scene must
 * live until they are done.  Image, accumulators, counters and every setting are kept. */
int vrc_renderer_set_scene(vrc_renderer *r, const vrc_scene *s);

/* One frame = what the swarm lambda does (main.cpp:139-152): for every selected
 * pixel, Camera::getRay + RayCaster::renderRay, `spp` times.  Adds to the
 * renderer's running vrc_frame_stats.  Asynchronous on `stream`. */
int vrc_render_frame(vrc_renderer *r, const vrc_camera *cam, const vrc_frame_params *p, void *stream);
/* vrc_render_frame followed by vrc_resolve_shard(r, p->row_block, p->shard_index, p->shard_count, dst_dev, reset = 1)
 * -- i.e. the swarm lambda, samples_to_image() and resetSamples() of one progressive frame (main.cpp:139-158,
 * raycaster.hpp:94-116) -- as ONE launch: the tile's last work unit turns the tile's sample sums into RGBA8 (into the
 * image and, if dst_dev != NULL, into the packed shard buffer) and leaves the accumulators at zero.  Needs
 * p->use_samples and accumulators that are zero on entry (after creation, vrc_reset_samples, vrc_resolve_shard(reset)
 * or a previous call of this function); same image, same shard rows, same counters as the two calls.  Rows of dst_dev
 * that correspond to no image row (padding of the last row block / slot) are left untouched.  Frame kernels or modes
 * that cannot fuse (checkerboard) run the two calls instead. */
int vrc_render_frame_resolved(vrc_renderer *r, const vrc_camera *cam, const vrc_frame_params *p, void *dst_dev, void *stream);
/* Optional: also record the primary-ray HitPoint of sample 0 per pixel into
 * prim_dev (device memory, width*height vrc_hit) during the next frames; NULL disables. */
int vrc_renderer_set_primary_capture(vrc_renderer *r, vrc_hit *prim_dev);

int vrc_samples_to_image(vrc_renderer *r, void *stream);  /* raycaster.hpp:94-103 */
int vrc_reset_samples(vrc_renderer *r, void *stream);     /* raycaster.hpp:105-116 */
int vrc_clear_image(vrc_renderer *r, void *stream);       /* render_image.create() again */

/* render_image (raycaster.hpp:261): RGBA8 row-major, width*height*4 bytes. */
void *vrc_image_device_ptr(vrc_renderer *r);              /* for device-side gathers (RCCL) */
void *vrc_accum_device_ptr(vrc_renderer *r);              /* uint32 r,g,b,count per pixel */
int vrc_read_image(vrc_renderer *r, uint8_t *rgba_host, void *stream);   /* synchronous */
int vrc_write_image(vrc_renderer *r, const uint8_t *rgba_host, void *stream); /* synchronous */
int vrc_read_accum(vrc_renderer *r, uint32_t *accum_host, void *stream);  /* synchronous */

/* Synchronises `stream`, returns and optionally clears the running stats. */
int vrc_get_stats(vrc_renderer *r, vrc_frame_stats *out, int reset, void *stream);

/* Direct peer writes (the alternative to a collective -- "direct peer writes into the root's framebuffer";
 * include/raycaster.hpp:84,261: the one render_image every swarm worker writes its pixels into).  The presenting process
 * exports the framebuffer of a renderer (vrc_ipc_export_image); every other process of the node opens it
 * (vrc_ipc_open_image) and makes it the target of its own renderer (vrc_renderer_set_image_target): a sharded
 * vrc_render_frame_resolved / vrc_resolve_shard then writes this shard's rows of the frame where they belong in the
 * presenter's memory -- over xGMI between GPUs -- instead of into the renderer's own image: no pack, no collective, no unpack.
 * Ordering between the processes is by FRAME FLAGS: 32-bit counters in a POSIX shared-memory segment (vrc_ipc_flags_open:
 * one process creates "/name", the others open it) that are written and waited for in stream order -- a writer sets "my
 * rows of frame n are in" behind its frame (vrc_stream_write_flag), the presenter's stream waits until the flag is >= n
 * (vrc_stream_wait_flag) before it reads the frame, and the other way round before a writer reuses a framebuffer.  A wait
 * names a value, so no host-side handshake is needed.  The image handle is 64 opaque bytes to pass by any host channel. */
typedef struct vrc_ipc_handle { unsigned char opaque[64]; } vrc_ipc_handle;
typedef struct vrc_ipc_flags vrc_ipc_flags;
int vrc_ipc_export_image(vrc_renderer *r, vrc_ipc_handle *out);
int vrc_ipc_open_image(int device, const vrc_ipc_handle *handle, void **image_dev);
int vrc_ipc_close_image(int device, void *image_dev);
/* image_dev: RGBA8 width x height of this renderer's size on any device this one can reach; NULL = the renderer's own image. */
int vrc_renderer_set_image_target(vrc_renderer *r, void *image_dev);
/* create = 1: makes the segment (zeros) and records this process as its owner; a segment of that name that already
 * exists is replaced only when its owner is gone (a run that died) -- one that is still in use is VRC_ERR_INVALID, so give
 * concurrent runs different names (a pid or a token in it).  create = 0: opens it; a segment that is smaller than `count`
 * asks for or was made for another count is VRC_ERR_INVALID, never a fault on first touch. */
int vrc_ipc_flags_open(const char *name, uint32_t count, int device, int create, vrc_ipc_flags **out);
/* Host-side store to a flag (release order; e.g. an "everyone may leave" word the processes poll with vrc_ipc_flag_value). */
int vrc_ipc_flag_set(vrc_ipc_flags *f, uint32_t index, uint32_t value);
/* A stream-ordered wait (vrc_stream_wait_flag) HAS NO TIMEOUT: if the process that should write the flag died, the stream --
 * and every hipStreamSynchronize on it -- waits for ever.  So a host never synchronises such a stream blindly; it calls
 * vrc_ipc_stream_wait: polls `stream` until everything enqueued on it has completed (VRC_OK), or until one of the peers
 * `pids` (process ids on this node, n_pids of them; may be NULL) no longer exists, or NO FLAG of the segment has changed for `timeout_ms` (an inactivity limit, not a deadline from the
 * start of the call: a healthy exchange that is still draining a long queue keeps moving its flags; 0 = no limit: only the
 * peers' disappearance ends the wait), or another process has already given up on this segment.  On those three it gives up for everyone: marks the segment and writes
 * 0xffffffff into every flag from the host, which releases every wait on them in every process, holds them there while the
 * stream drains (the flag writes still queued behind the waits would lower them again) and returns VRC_ERR_PEER; call it for
 * every stream of the process before leaving, so that no wait stays pending on the device (frames completed after that are not valid; vrc_stream_wait_flag / _write_flag on a marked segment
 * fail with VRC_ERR_PEER as well).  Start a fresh process to try again. */
int vrc_ipc_stream_wait(vrc_ipc_flags *f, void *stream, const int32_t *pids, uint32_t n_pids, uint32_t timeout_ms);
/* The creator removes the segment's NAME once every process of the run has opened it (the caller's barrier says when): the
 * mappings stay valid, and a run that is killed afterwards leaves nothing behind in /dev/shm. */
int vrc_ipc_flags_unlink(vrc_ipc_flags *f);
int vrc_ipc_flags_close(vrc_ipc_flags *f);                     /* the creator also removes the name, if it has not yet */
int vrc_stream_write_flag(vrc_ipc_flags *f, uint32_t index, uint32_t value, void *stream);
int vrc_stream_wait_flag(vrc_ipc_flags *f, uint32_t index, uint32_t value, void *stream);      /* until flag >= value */
uint32_t vrc_ipc_flag_value(const vrc_ipc_flags *f, uint32_t index);                           /* host read */

/* Multi-GPU frame sharding: compact this shard's row blocks into
 * `dst_dev` (ceil(nblocks/shard_count) blocks of row_block*width*4 bytes), and
 * the inverse scatter of an all-gathered buffer [shard][slot] into a full frame. */
uint64_t vrc_shard_bytes(uint32_t width, uint32_t height, uint32_t row_block, uint32_t shard_count);
int vrc_pack_shard(vrc_renderer *r, uint32_t row_block, uint32_t shard_index, uint32_t shard_count,
                   void *dst_dev, void *stream);
/* vrc_samples_to_image + vrc_pack_shard (+ vrc_reset_samples when `reset` != 0) for this shard's row blocks in
 * one pass: resolves the accumulators of the shard's pixels into the image and, when dst_dev != NULL, into the
 * packed shard buffer; with `reset` the same pixels' accumulators are zeroed for the next frame (a following
 * vrc_render_frame must be ordered after this call, as it would after vrc_reset_samples).
 * shard_count == 1 with row_block == 0 covers the whole frame (dst_dev layout == image layout). */
int vrc_resolve_shard(vrc_renderer *r, uint32_t row_block, uint32_t shard_index, uint32_t shard_count,
                      void *dst_dev, int reset, void *stream);
/* Launches on the device that owns image_dev. */
int vrc_unpack_shards(const void *gathered_dev, uint32_t width, uint32_t height, uint32_t row_block,
                      uint32_t shard_count, void *image_dev, void *stream);

/* ---- post-process / present chain that follows the path (main.cpp:160-182) ---------- */

/* Device-resident restatement of what main.cpp does with render_image every frame, so that the frame stays in
 * HBM between the renderer and whatever shows it (no PCIe read-back):
 *   render_tex   = render_image x Color(255 * (1 - old))                        (sf::BlendMultiply, :163-172)
 *   denoised_tex = denoised_tex x Color(255 * old) + render_tex, saturating     (BlendMultiply, BlendAdd, :161-162,175-177)
 *   window       = denoised_tex scaled to out_width x out_height, nearest       (final_sprite.setScale(1 / 0.75), :179-182)
 * with old = old_value_conservation (main.cpp:161: use_samples ? 0 : 0.1), and an optional per-channel median around
 * the sampled texel: median = 0 none, 3 = the 3x3 network of res/median_3.frag, 5 = the 5x5 network of
 * res/median.frag as shipped (taps one texel apart, clamped to the edge).  UNORM8 products are rounded to nearest,
 * round(a * b / 255) -- fixed-function GL blending is not specified bit-exactly, so against a real GL device the two
 * blend steps carry a tolerance of +-1 LSB each; upscale and median are exact.  The presenter owns denoised_tex
 * (zero at creation, persistent across frames) and the window image. */
typedef struct vrc_presenter vrc_presenter;
int vrc_presenter_create(int device, uint32_t width, uint32_t height, uint32_t out_width, uint32_t out_height,
                         vrc_presenter **out);
int vrc_presenter_destroy(vrc_presenter *p);
/* One frame of the chain on the renderer's framebuffer (same device, same size).  Asynchronous on `stream`. */
int vrc_present(vrc_presenter *p, vrc_renderer *r, float old_value_conservation, uint32_t median, void *stream);
/* The same on any device-resident RGBA8 image of the presenter's render size (e.g. a gathered multi-GPU frame). */
int vrc_present_image(vrc_presenter *p, const void *image_dev, float old_value_conservation, uint32_t median, void *stream);
int vrc_presenter_clear(vrc_presenter *p, void *stream);          /* denoised_tex = 0 */
void *vrc_presenter_window_ptr(vrc_presenter *p);                 /* RGBA8 out_width x out_height, device */
void *vrc_presenter_denoised_ptr(vrc_presenter *p);               /* RGBA8 width x height, device */
/* Copies the window image and / or denoised_tex to host memory (either may be NULL).  Synchronous.  `stream` must be the
 * stream of the vrc_present call whose result is wanted (or one ordered after it): streams made by vrc_stream_create are
 * non-blocking, so a read on the NULL stream does not wait for a present issued on one of them. */
int vrc_presenter_read(vrc_presenter *p, uint8_t *window_rgba_host, uint8_t *denoised_rgba_host, void *stream);

/* Self-test of the arithmetic shortcuts: the kernels compute -1 / |d| (lsvo.hpp:47), glm::normalize's 1 / sqrt and
 * getRand's x / 100 (utils.cpp:77-81) by v_rcp_f32 / v_rsq_f32 + one FMA correction step where that is proven equal to
 * the correctly rounded IEEE result, and by the IEEE expansion elsewhere.  This runs the proof on `device`: every float
 * bit pattern of the ranges concerned against the IEEE operations.  mismatches[0..3] = reciprocal, square root,
 * 1 / sqrt, get_rand; all zero on a conforming device. */
int vrc_selftest_exact_arith(int device, uint64_t mismatches[4]);

/* Host helper: generateRotationMatrix (utils.cpp:94-100) for Camera::setViewAngle. */
void vrc_make_rotation(float angle_x, float angle_y, float rot[9]);

/* Scheduling knobs.  vrc_set_* change the process-wide DEFAULTS that new renderers copy at
 * creation (thread-safe); vrc_renderer_set_* change one renderer (a renderer is not re-entrant,
 * so call them between its frames).  Results never depend on them.
 * blocks_per_cu: resident 256-thread workgroups of the frame kernel per CU (= waves per SIMD),
 * 0 = the library's choice, at most 8 -- see vrc_renderer_last_kernel below for the builds. */
int vrc_set_tuning(uint32_t blocks_per_cu);
/* Sample mode: samples per work unit (tile x sample chunk).  0 =
 * automatic: the largest chunk that still gives every wave a few dozen units (down to 1 sample
 * per unit for small multi-GPU shards), and half that chunk for the tiles handed out last, so
 * that units get shorter towards the end of a launch; a pixel's samples split over several
 * units are accumulated with integer atomics (same sums).  Values >= 0xffff0000 set the
 * automatic mode's tail policy instead: low 16 bits = units per wave with the halved chunk. */
int vrc_set_sample_chunk(uint32_t samples_per_unit);
/* The stage-synchronous kernel is built for 6 resident workgroups per CU (= waves per SIMD) and, for
 * cameras with a lens, also for 7; the library picks by the kind of launch (csrc/vrc_plan.h,
 * plan_frame), and blocks_per_cu >= 7 picks the 7-wave build where there is one (fewer than 6:
 * the 6-wave build on fewer workgroups).
 * vrc_renderer_last_kernel: the symbol of the frame kernel the renderer's last frame launched
 * (what a profile of the run lists), "" before the first frame. */
const char *vrc_renderer_last_kernel(const vrc_renderer *r);
int vrc_renderer_set_tuning(vrc_renderer *r, uint32_t blocks_per_cu);
int vrc_renderer_set_sample_chunk(vrc_renderer *r, uint32_t samples_per_unit);
/* Beyond the reference (off by default).  With aperture exactly +0 -- the reference's default
 * camera -- a pixel's primary ray and the shadow ray(s) of its hit are the same for every
 * sample, and RayCaster::renderRay (raycaster.hpp:119-167) walks them again each time.  on = 1
 * lets the stage-synchronous kernel walk them ONCE per work unit (tile x sample chunk: once per
 * pixel and frame with vrc_renderer_set_sample_chunk(r, spp)) and share the result between the
 * unit's samples; the GI rays stay per sample.  Image, accumulators and primary capture are bit
 * for bit the same; vrc_frame_stats.rays / sum_complexity then count the walks EXECUTED, i.e.
 * fewer than the reference's.  No effect with aperture != 0. */
int vrc_renderer_set_invariant_ray_reuse(vrc_renderer *r, uint32_t on);
/* Measurement / A-B switch (off by default): on = 1 makes the frame kernel start EVERY ray at the
 * root, as lsvo.hpp:60-72 does, instead of below it next to the previous hit / the camera
 *  -- for every kind of frame (pinhole or lens, one bounce or the 2-bounce
 * extension; the builds of the 8 x 8 lane map at 6 waves per SIMD, vrc_renderer_last_kernel ends in
 * "_from_root").  Same image, same vrc_frame_stats.rays / sum_complexity either way;
 * iterations_not_executed is 0 with it.  (bench.py reports the frame time with it as
 * extra.every_ray_from_the_root.) */
int vrc_renderer_set_walk_from_root(vrc_renderer *r, uint32_t on);
/* The lane <-> (pixel, sample) map of the stage-synchronous kernel.  The reference's own map of
 * pixels to workers is the static 4 x 4 area grid of main.cpp:140-143; results do not depend on
 * it there or here.  samples = 1: a wave takes 8 x 8 pixels and loops over the samples of its work
 * unit.  samples = 4: a wave takes 4 x 4 pixels with four samples of each side by side (the four
 * lanes of a pixel share its primary hit: a stage's longest ray is the longest of 16 neighbouring
 * pixels', not of 64) -- for sample-mode frames (use_samples) with spp a multiple of 4, one GI
 * bounce and no checkerboard; other frames use map 1 whatever is set.  samples = 0 (default): the
 * library's choice -- four abreast for a launch that has the chip to itself (3-6 % off a frame's
 * latency), the pixel tiles for whole-spp work units (vrc_renderer_set_sample_chunk(r, spp): frames
 * in flight, where they are 5 % faster).  Image, accumulators, captures and vrc_frame_stats are the
 * same either way. */
int vrc_renderer_set_lane_samples(vrc_renderer *r, uint32_t samples);
int vrc_set_lane_samples(uint32_t samples);                 /* the process default new renderers copy */
/* Quadrant walks (round 5; on by default).  With a pinhole camera a pixel's primary ray and the
 * shadow ray of its hit are the same for every sample, and the reference walks them once per sample
 * (raycaster.hpp:131,153).  on = 1: where a launch allows it the pinhole kernels lay those walks out
 * as one quadrant of the 8 x 8 tile at a time, 16 pixels with their four samples side by side in the
 * wave, instead of 64 pixels with one sample -- every ray is still walked, each by its own lane, but a
 * stage lasts as long as the longest ray of 16 neighbouring pixels instead of 64 (C3: 6.5 % fewer
 * instructions, 5.5 % less time; 16 spp: 11 %).  Applies to sample-mode frames on the 8 x 8 lane map whose work
 * units all have a multiple of four samples (spp and the sample chunk multiples of four), without
 * invariant-ray reuse and primary-hit capture, on trees of 8 levels or more; every other launch runs
 * the plain kernels (vrc_renderer_last_kernel ends in "_q" when it applied).  on = 0: never.  Image,
 * accumulators and vrc_frame_stats are the same either way. */
int vrc_renderer_set_quad_walks(vrc_renderer *r, uint32_t on);

#ifdef __cplusplus
}
#endif
#endif
