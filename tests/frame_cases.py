"""Scenes, poses and oracle frames shared by tests/test_frame_cases_host.py (no GPU: are the cases worth rendering?) and
tests/test_gpu_frame_builds.py (the _q, _s4 and _w7 builds of the frame kernel against the oracle on exactly these cases).

Scenes are voxel lists compiled by the oracle's restated setCell + compileSVO (oracle_lib.compile_voxels): every leaf is a unit
voxel.  An object is 80 voxels wide and centred at S/2, so the same generator serves every depth from 7 up and the frame looks
the same at each.  The walk sees what setCell stored point-reflected (slot = idx ^ mirror_mask, lsvo.hpp:79): a voxel stored at
(x, y, z) is met by rays at S - 1 - (x, y, z).  The generators below speak of the coordinates the RAYS see -- `seen` -- and
reflect once, at the end.

Poses are (position in voxels, yaw, pitch, fov, aperture, focal_length); lights are positions in SVO space ([1, 2)^3 is the
volume), as RayCaster.setLightPosition takes them."""
import collections

import numpy as np

import oracle_lib as O
from cpuvoxelraycaster_amd.scenes import reference_light

Pose = collections.namedtuple("Pose", "position yaw pitch fov aperture focal_length")

# tests/test_gpu_start_below.py::test_light_anywhere: 1e30 away (the direction collapses to +-EPS), inside the volume, on a plane
LIGHTS_ANYWHERE = ((3e29, -8e29, 1e30), (1e19, 1e19, -1e19), (1.31, 1.62, 1.4), (1.5, 1.75, 1.25), (-40.0, 900.0, 12.0))
FAR_LIGHT = LIGHTS_ANYWHERE[0]
SCENES = ("bowl", "lattice")                      # (and "shell", the closed bowl, and "random" for shallow trees)
BASE_SIZE = (72, 40)


def light_of(depth, which=None):
    """None = the reference's light scaled to the scene (main.cpp:124-126), else an index into LIGHTS_ANYWHERE"""
    return tuple(float(v) for v in (reference_light(depth) if which is None else np.asarray(LIGHTS_ANYWHERE[which], np.float32)))


# ---- scenes ----

def bowl_offsets():
    """an open bowl: a spherical shell of radius 40, 3 voxels thick, without its cap on the light's side (-y, where the
    cameras are too), and 3000 scattered voxels in its bounding box; offsets from the centre, as the rays see them"""
    g = np.indices((81, 81, 81)).reshape(3, -1).T.astype(np.int64) - 40
    r2 = (g * g).sum(1)
    shell = g[(r2 <= 40 * 40) & (r2 > 37 * 37) & (g[:, 1] > -24)]
    debris = np.random.default_rng(40).integers(-40, 40, (3000, 3))
    return np.concatenate([shell, debris])


def shell_offsets():
    """the bowl closed and empty: whoever is inside sees no light, wherever the light is (docs/NOTEBOOK.md)"""
    g = np.indices((81, 81, 81)).reshape(3, -1).T.astype(np.int64) - 40
    r2 = (g * g).sum(1)
    return g[(r2 <= 40 * 40) & (r2 > 37 * 37)]


def lattice_offsets():
    """walls and pillars one voxel thick with gaps, a slab behind them and overhangs; offsets from the centre, as seen"""
    a = np.arange(-40, 40)
    u, v = [m.reshape(-1) for m in np.meshgrid(a, a, indexing="ij")]
    parts = []
    for x in (-31, -9, 13, 35):                                # walls across x, windows 5 of every 12 voxels each way
        keep = ((u % 12) >= 5) | ((v % 12) >= 5)
        parts.append(np.stack([np.full(keep.sum(), x), u[keep], v[keep]], 1))
    for z in (-22, 17):                                        # walls across z, every third 8 x 8 panel missing
        keep = ((u // 8 + v // 8) % 3) != 0
        parts.append(np.stack([u[keep], v[keep], np.full(keep.sum(), z)], 1))
    px, pz = [m.reshape(-1) for m in np.meshgrid(np.arange(-38, 40, 7), np.arange(-38, 40, 11), indexing="ij")]
    for x, z in zip(px, pz):                                   # pillars along y, one voxel thick, broken off at different heights
        y = np.arange(-40 + (x * 5 + z * 3) % 23, 40)
        parts.append(np.stack([np.full(len(y), x), y, np.full(len(y), z)], 1))
    slab = (v % 16 != 7)                                       # the slab (three voxels, far side) with slits
    for y in (30, 31, 32):
        parts.append(np.stack([u[slab], np.full(slab.sum(), y), v[slab]], 1))
    for y, x0, z0 in ((-12, -31, -30), (-2, 13, -5), (9, -9, 10)):   # overhangs: plates that stick out of a wall over empty space
        ox, oz = [m.reshape(-1) for m in np.meshgrid(np.arange(x0, x0 + 14), np.arange(z0, z0 + 22), indexing="ij")]
        parts.append(np.stack([ox, np.full(len(ox), y), oz], 1))
    return np.unique(np.concatenate(parts), axis=0)


def random_volume(depth):
    """trees shallower than the objects: a random volume, denser in its far half, as test_shallow_and_deep_trees has it, but
    thinned with the size (about 1 and 3 solid voxels along an axis-parallel line) so that some camera rays get through and
    light gets in; solid[x, y, z] as the rays see it"""
    rng = np.random.default_rng(depth)
    S = 1 << depth
    vol = rng.random((S, S, S)) < min(0.3, 1.0 / S)
    vol[:, S // 2:, :] |= rng.random((S, S - S // 2, S)) < min(0.5, 2.0 / S)
    return vol


_NODES = {}


def scene_nodes(name, depth):
    """the LNode array of a scene (compiled once per process)"""
    if (name, depth) not in _NODES:
        S = 1 << depth
        if name == "random":
            vox = (S - 1) - np.argwhere(random_volume(depth)).astype(np.int64)
        else:
            assert S >= 128, "the objects are 80 voxels wide"
            seen = {"bowl": bowl_offsets, "lattice": lattice_offsets, "shell": shell_offsets}[name]() + S // 2
            vox = (S - 1) - seen                                # what setCell must store for the rays to see `seen`
        _NODES[(name, depth)] = O.compile_voxels(depth, vox)
    return _NODES[(name, depth)]


# ---- poses ----

def svo_position(pose, depth):
    """the camera position in SVO space as the kernels and the oracle compute it (main.cpp:149)"""
    f = np.float32
    return (np.asarray(pose.position, f) * (f(1.0) / f(1 << depth)) + f(1.0)).astype(f)


def oracle_camera(pose):
    return O.make_camera(pose.position, O.make_rotation(pose.yaw, pose.pitch), pose.fov, pose.aperture, pose.focal_length)


def lens(pose, aperture=0.4):
    """the same pose through a lens focused about where the object is"""
    return pose._replace(aperture=aperture, focal_length=60.0)


_POSES = {}


def poses(name, depth):
    """{"a": general position, "b": on the centre planes x = z = 1.5, "c": along an axis with a wide field, on the plane
    x = 1.5, "d": inside a solid voxel}"""
    if (name, depth) in _POSES:
        return _POSES[(name, depth)]
    S = float(1 << depth)
    h = S / 2
    if name == "random":
        # in the empty voxel of the near face (y = 0) that is closest to the face's middle, off its centre, looking inwards
        empty = np.argwhere(~random_volume(depth)[:, 0, :])
        x, z = empty[np.argmin(((empty - (h - 0.5)) ** 2).sum(1))]
        out = {"a": Pose((x + 0.63, 0.21, z + 0.37), 0.4, -0.8, 0.8, 0.0, S / 2)}
    elif name == "shell":
        out = {"e": Pose((h + 3.3, h + 10.2, h - 5.1), 0.3, -1.3, 1.0, 0.0, 1.0)}      # enclosed
    elif name == "bowl":
        out = {"a": Pose((h + 0.5, h - 70.2, h + 0.5), 0.3, -1.3, 1.0, 0.0, 1.0),
               "b": Pose((h, h - 66.0, h), -0.8, -1.15, 0.9, 0.0, 1.0),
               # the axis +z lies inside the frame, 1.8 pixels right of and below its centre: the x and the y component change sign
               # there, and the quadrant at (36, 20) holds four mirror masks, four pixels each
               "c": Pose((h, h - 8.3, h - 61.6), -0.1, 0.1, 0.45, 0.0, 1.0)}
    else:
        out = {"a": Pose((h + 4.3, h - 75.6, h - 6.4), 0.5, -1.2, 1.0, 0.0, 1.0),
               "b": Pose((h, h - 68.0, h), 2.4, -1.0, 0.8, 0.0, 1.0),
               "c": Pose((h, h + 5.3, h - 64.6), -0.1, 0.1, 0.45, 0.0, 1.0)}
    if name in SCENES:
        # (d): the centre of the solid voxel that the central ray of pose (a) hits
        a = out["a"]
        rot = O.make_rotation(a.yaw, a.pitch).reshape(3, 3)
        d = (rot @ np.array([0.0, 0.0, 1.0], np.float32)).astype(np.float32)
        hit = O.cast_rays(scene_nodes(name, depth), depth, svo_position(a, depth)[None], d[None], 0.0, 0.0)[0]
        assert hit["hit"] != 0
        p = (hit["position"].astype(np.float64) - 1.0) * S - 0.5 * np.sign(hit["normal"].astype(np.float64))
        out["d"] = Pose(tuple(float(np.floor(c) + 0.5) for c in p), a.yaw, a.pitch, 1.0, 0.0, 1.0)
    _POSES[(name, depth)] = out
    return out


def mirror_masks(pose, W, H):
    """(H, W) direction-sign masks of a pinhole pose's camera rays (bit i: component i > 0), in float64: which tiles mix masks"""
    rot = O.make_rotation(pose.yaw, pose.pitch).reshape(3, 3).astype(np.float64)
    y, x = np.indices((H, W)).astype(np.float64)
    v = np.stack([x / H - (W / H) * 0.5, y / H - 0.5, np.full((H, W), pose.fov)], -1)
    d = v @ rot.T
    return (d[..., 0] > 0) * 1 + (d[..., 1] > 0) * 2 + (d[..., 2] > 0) * 4


# ---- oracle frames, shared by every test that asks for the same one ----

Frame = collections.namedtuple("Frame", "accum prim rays steps hits")
_FRAMES = {}


def oracle_frame(name, depth, pose, light, spp, shadows=1, bounces=1, size=BASE_SIZE, frame=0, shard=(0, 0, 1), textures=None):
    """the samples frame * spp .. frame * spp + spp - 1 summed by orc_render_frame: accumulators, the primary HitPoints of the
    first of them, rays, loop iterations and primary hits over all of them.  Read-only: callers must not write into it."""
    key = (name, depth, tuple(pose), tuple(light), spp, shadows, bounces, tuple(size), frame, tuple(shard))
    if key not in _FRAMES:
        top, side = textures if textures is not None else O.load_textures()
        W, H = size
        cam = oracle_camera(pose)
        acc, first, rays, steps, hits = None, None, 0, 0, 0
        for s in range(spp):
            p = O.make_params(W, H, light, use_gi=1, use_samples=1, shadow_samples=shadows, gi_bounces=bounces, frame_index=frame * spp + s,
                              row_block=shard[0], shard_index=shard[1], shard_count=shard[2])
            _, acc, prim, st = O.render_frame(scene_nodes(name, depth), depth, top, side, cam, p, accum=acc, want_prim=True, threads=8)
            first = prim if s == 0 else first
            rays, steps, hits = rays + st.rays, steps + st.sum_complexity, hits + st.primary_hits
        acc.setflags(write=False)
        first.setflags(write=False)
        _FRAMES[key] = Frame(acc, first, rays, steps, hits)
    return _FRAMES[key]


# ---- what the GPU tests render: tests/test_frame_cases_host.py holds every one of these views to its conditions ----

ENCLOSED_LIGHT = (1.52, 1.45, 1.49)                                   # inside the shell
BASE_DEPTH = 8
BASE_VIEWS = [(name, BASE_DEPTH, k) for name in SCENES for k in "abc"]    # (scene, depth, pose)
DEEP_VIEWS = [("bowl", 10, "a"), ("bowl", 11, "a")]
SHALLOW_VIEWS = [("random", d, "a") for d in (2, 3, 4, 6)]
SOLID_VIEWS = [(name, BASE_DEPTH, "d") for name in SCENES]
LIGHT_VIEW = ("bowl", BASE_DEPTH, "a")                                # under each of LIGHTS_ANYWHERE
SHADOW_VIEW = ("lattice", BASE_DEPTH, "a")                            # with 0 (= the reference's 4) and 2 shadow samples
SIZE_VIEW = ("lattice", BASE_DEPTH, "c")                              # at 17 x 9 and 7 x 5
SHARD_VIEW = ("lattice", BASE_DEPTH, "b")
ENCLOSED_VIEW = ("shell", BASE_DEPTH, "e")
SMALL_SIZES = ((17, 9), (7, 5))
