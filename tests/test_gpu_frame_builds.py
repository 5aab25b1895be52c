"""The builds of the frame kernel that the library runs by default -- _q (quadrant walks), _s4 (four samples abreast), _w7 (the
lens kernel with whole-spp units) -- against orc_render_frame under the conditions only the plain 8 x 8 builds had met
(tests/test_gpu_start_below.py): cameras off the grid planes, on them, and at a meeting of four mirror masks; a camera inside
a solid voxel; lights anywhere; thin walls, overhangs and debris instead of a heightfield; trees of depth 2..4, 6, 10 and 11;
frames smaller than a tile; a shard.  Scenes, poses and the (cached) oracle frames come from tests/frame_cases.py, and
tests/test_frame_cases_host.py proves without a GPU that these views are worth rendering.

Every case forces a build, asserts lastKernel() and compares accumulators or image, rays, loop iterations, primary hits and --
where the build allows a capture -- every primary HitPoint byte for byte.  When a comparison fails, the same case is rendered
once more by the plain build and with every ray from the root, and the failure says which of the three disagree with the
oracle: the build under test alone = its lane map, plain too = the start below the root, all three = the oracle or the case."""
import numpy as np
import pytest

import frame_cases as F

pytestmark = pytest.mark.gpu

_SVO = {}


def svo_of(vrc, textures, name, depth):
    if (name, depth) not in _SVO:
        _SVO[(name, depth)] = vrc.LSVO(F.scene_nodes(name, depth), depth, textures=textures)
    return _SVO[(name, depth)]


def symbol(family, pose, bounces, fused):
    res = "_resolved" if fused else ""
    if family in ("q", "plain_pinhole"):
        return "k_render_sync_pinhole" + ("2" if bounces == 2 else "") + res + ("_q" if family == "q" else "")
    if family == "s4":
        return "k_render_sync" + ("_pinhole" if pose.aperture == 0.0 else "") + res + "_s4"
    return "k_render_sync" + res + "_w7"


def render(vrc, svo, textures, family, view, pose, light, spp, chunk, shadows, bounces, size, fused, frames, shard):
    """renders `frames` consecutive frames with the build `family` forces; returns (mismatches against the oracle, kernel, stats)"""
    import torch
    name, depth, _ = view
    W, H = size
    rc = vrc.RayCaster(svo, (W, H))
    rc.setLightPosition(light)
    rc.use_gi, rc.use_samples, rc.shadow_samples, rc.gi_bounces = True, True, shadows, bounces
    capture = family != "q"                                   # (the quadrant walks do not run under a capture: vrc_plan.h)
    if family == "q":
        rc.setLaneSamples(1)
        rc.setSampleChunk(chunk)
    elif family == "s4":
        rc.setLaneSamples(4)
    elif family == "w7":
        rc.setLaneSamples(1)
        rc.setSampleChunk(spp)
    else:                                                     # the yardsticks of a failure: "plain", "from_root"
        rc.setLaneSamples(1)
        rc.setQuadWalks(False)
        rc.setWalkFromRoot(family == "from_root")
    prim = None
    if capture:
        prim = torch.zeros(W * H * 48, dtype=torch.uint8, device="cuda")
        rc.setPrimaryCapture(prim.data_ptr())
    cam = vrc.make_camera(pose.position, F.O.make_rotation(pose.yaw, pose.pitch), pose.fov, pose.aperture, pose.focal_length)
    RB, k, N = shard
    own = ((np.arange(H) // RB) % N == k) if RB else np.ones(H, bool)
    bad, acc_sum, rays, steps, hits = [], 0, 0, 0, 0
    for frame in range(frames):
        assert rc.frame_index == frame * spp
        if fused:
            rc.renderFrameResolved(cam, spp=spp, row_block=RB, shard_index=k, shard_count=N)
        else:
            rc.renderFrame(cam, spp=spp, row_block=RB, shard_index=k, shard_count=N)
        torch.cuda.synchronize()
        ref = F.oracle_frame(name, depth, pose, light, spp, shadows, bounces, size, frame, shard, textures)
        rays, steps, hits = rays + ref.rays, steps + ref.steps, hits + ref.hits
        if fused:
            if not np.array_equal(rc.readImage()[own], F.O.samples_to_image(ref.accum)[own]):
                bad.append(f"image of frame {frame}")
            if rc.readAccum().any():
                bad.append(f"accumulators not reset after frame {frame}")
        else:
            acc_sum = acc_sum + ref.accum                     # renderFrame adds to what the accumulators hold
            if not np.array_equal(rc.readAccum(), acc_sum):
                bad.append(f"accumulators after frame {frame}")
        if capture and np.frombuffer(prim.cpu().numpy().tobytes(), dtype=vrc.HIT_DTYPE).tobytes() != ref.prim.tobytes():
            bad.append(f"primary capture of frame {frame}")
    st = rc.stats()
    for what, got, want in (("rays", st.rays, rays), ("sum_complexity", st.sum_complexity, steps), ("primary_hits", st.primary_hits, hits)):
        if got != want:
            bad.append(f"{what} {got} != {want}")
    kernel = rc.lastKernel()
    rc.setPrimaryCapture(None)
    rc.close()
    return bad, kernel, st


def check(vrc, textures, family, view, spp, chunk=None, shadows=1, bounces=1, size=F.BASE_SIZE, fused=False, frames=1, shard=(0, 0, 1),
          light=None, aperture=0.0, expect=None):
    name, depth, k = view
    pose = F.poses(name, depth)[k]
    if aperture:
        pose = F.lens(pose, aperture)
    light = F.light_of(depth) if light is None else light
    svo = svo_of(vrc, textures, name, depth)
    args = (view, pose, light, spp, chunk, shadows, bounces, size, fused, frames, shard)
    bad, kernel, st = render(vrc, svo, textures, family, *args)
    expect = expect or (symbol(family, pose, bounces, fused),)
    assert kernel in expect, (kernel, expect)
    if bad:                                                   # once, to be read: who else disagrees with the oracle?
        others = {alt: render(vrc, svo, textures, alt, *args)[0] for alt in ("plain", "from_root")}
        raise AssertionError(f"{kernel} differs from the oracle in {bad}; the plain build in {others['plain'] or 'nothing'}; "
                             f"every ray from the root in {others['from_root'] or 'nothing'}")
    if k == "a" and depth >= 3:                               # (the views whose camera path ends below the root: test_frame_cases_host.py)
        assert st.iterations_not_executed > 0
    return st


@pytest.fixture(scope="module")
def ctx(built, textures):
    import cpuvoxelraycaster_amd as vrc
    return vrc, textures


# ---- both scenes x poses (a), (b), (c) under the reference's light, depth 8 ----

VIEWS = [pytest.param(v, id="-".join(map(str, v))) for v in F.BASE_VIEWS]


@pytest.mark.parametrize("spp,chunk", [(4, 4), (8, 8), (16, 16), (8, 4)])          # 4, 8, 16 and 4 lanes per pixel
@pytest.mark.parametrize("view", VIEWS)
def test_quadrant_walks(ctx, view, spp, chunk):
    fused = (F.BASE_VIEWS.index(view) + (spp + chunk) // 8) % 2 == 0                 # both resolves on every view
    check(*ctx, "q", view, spp, chunk=chunk, fused=fused, frames=2 if spp == 4 else 1)


@pytest.mark.parametrize("spp,aperture", [(4, 0.0), (4, 0.4), (8, 0.0), (8, 0.4)])
@pytest.mark.parametrize("view", VIEWS)
def test_four_samples_abreast(ctx, view, spp, aperture):
    fused = (spp // 4 + F.BASE_VIEWS.index(view) + (aperture > 0)) % 2 == 0
    check(*ctx, "s4", view, spp, aperture=aperture, fused=fused, frames=2 if spp == 4 else 1)


@pytest.mark.parametrize("spp", [3, 4])
@pytest.mark.parametrize("view", VIEWS)
def test_lens_kernel_at_seven_waves(ctx, view, spp):
    check(*ctx, "w7", view, spp, aperture=0.4, fused=(spp + F.BASE_VIEWS.index(view)) % 2 == 0, frames=2)


# ---- deep trees: the final state of a quadrant walk waits in rows 3..7 of a column that has exactly `depth` rows ----

@pytest.mark.parametrize("depth,bounces,fused", [(10, 1, True), (11, 1, False), (11, 2, True)])
def test_quadrant_walks_deep_trees(ctx, depth, bounces, fused):
    check(*ctx, "q", ("bowl", depth, "a"), 4, chunk=4, bounces=bounces, fused=fused, frames=2)


@pytest.mark.parametrize("depth,aperture,fused", [(10, 0.0, True), (10, 0.4, False), (11, 0.0, False), (11, 0.4, True)])
def test_four_samples_abreast_deep_trees(ctx, depth, aperture, fused):
    check(*ctx, "s4", ("bowl", depth, "a"), 4, aperture=aperture, fused=fused, frames=2)


def test_lens_kernel_deep_tree(ctx):
    """at depth 10 the stacks of seven workgroups may not fit a CU's LDS: then the planner falls back (plan_units: v.waves > fit),
    and its choice is accepted"""
    check(*ctx, "w7", ("bowl", 10, "a"), 4, aperture=0.4, fused=True, frames=2, expect=("k_render_sync_resolved_w7", "k_render_sync_resolved"))


# ---- shallow trees ----

@pytest.mark.parametrize("depth", [2, 3, 4, 6])
def test_quadrant_walks_need_eight_levels(ctx, depth):
    """below depth 8 a launch that asks for the quadrant walks runs the plain build (and still equals the oracle)"""
    fused = depth % 2 == 0
    check(*ctx, "q", ("random", depth, "a"), 4, chunk=4, fused=fused, expect=(symbol("plain_pinhole", None, 1, fused),))


@pytest.mark.parametrize("depth", [2, 3, 4, 6])
def test_four_samples_abreast_shallow_trees(ctx, depth):
    check(*ctx, "s4", ("random", depth, "a"), 4, aperture=0.0 if depth % 2 else 0.4, fused=depth >= 4, frames=2)


def test_lens_kernel_shallow_tree(ctx):
    check(*ctx, "w7", ("random", 4, "a"), 4, aperture=0.4, frames=2)


# ---- the light anywhere: 1e30 away (its direction collapses to +-EPS: an LOD ray must start at the root), inside, on a plane ----

@pytest.mark.parametrize("which", range(len(F.LIGHTS_ANYWHERE)))
def test_quadrant_walks_light_anywhere(ctx, which):
    check(*ctx, "q", F.LIGHT_VIEW, 4, chunk=4, light=F.light_of(F.BASE_DEPTH, which), bounces=1 + which % 2, fused=which in (2, 3))


@pytest.mark.parametrize("which", range(len(F.LIGHTS_ANYWHERE)))
def test_four_samples_abreast_light_anywhere(ctx, which):
    check(*ctx, "s4", F.LIGHT_VIEW, 4, light=F.light_of(F.BASE_DEPTH, which), aperture=0.4 * (which % 2), fused=which >= 3)


@pytest.mark.parametrize("which", [0, 2])
def test_lens_kernel_light_anywhere(ctx, which):
    check(*ctx, "w7", F.LIGHT_VIEW, 4, light=F.light_of(F.BASE_DEPTH, which), aperture=0.4, fused=which == 0)


# ---- a camera inside a solid voxel: t = 0 hits with an all-zero normal, a NaN GI direction ----

@pytest.mark.parametrize("family", ["q", "s4", "w7"])
@pytest.mark.parametrize("view", [pytest.param(v, id=v[0]) for v in F.SOLID_VIEWS])
def test_camera_inside_a_solid_voxel(ctx, view, family):
    fused = view[0] == "bowl"
    check(*ctx, family, view, 4, chunk=4, aperture=0.4 if family == "w7" else 0.0, fused=fused, bounces=2 if (family, fused) == ("q", False) else 1)


# ---- shadow samples: 0 = the reference's 4 (16 lanes per pixel in the quadrant shadow walks), and 2 ----

@pytest.mark.parametrize("shadows", [0, 2])
@pytest.mark.parametrize("family", ["q", "s4"])
def test_shadow_samples_on_the_lattice(ctx, family, shadows):
    check(*ctx, family, F.SHADOW_VIEW, 4, chunk=4, shadows=shadows, aperture=0.4 if (family, shadows) == ("s4", 2) else 0.0, fused=shadows == 2)


# ---- frames smaller than a tile row, smaller than a tile ----

@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("size", F.SMALL_SIZES)
@pytest.mark.parametrize("family", ["q", "s4", "w7"])
def test_small_frames(ctx, family, size, fused):
    check(*ctx, family, F.SIZE_VIEW, 4, chunk=4, size=size, fused=fused, frames=2, aperture=0.4 if family == "w7" else 0.0)


# ---- one shard of three, against the oracle with the same shard fields ----

@pytest.mark.parametrize("family,fused", [("q", True), ("s4", False)])
def test_sharded(ctx, family, fused):
    check(*ctx, family, F.SHARD_VIEW, 4, chunk=4, fused=fused, frames=2, shard=(8, 1, 3))


def test_enclosed_view(ctx):
    """black by construction (tests/test_frame_cases_host.py): compared on counters, and on the capture by the _s4 build"""
    check(*ctx, "q", F.ENCLOSED_VIEW, 4, chunk=4, light=F.ENCLOSED_LIGHT, fused=True)
    check(*ctx, "s4", F.ENCLOSED_VIEW, 4, light=F.ENCLOSED_LIGHT)
