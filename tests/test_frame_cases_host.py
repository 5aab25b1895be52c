"""The guard against vacuous parity of tests/test_gpu_frame_builds.py: every (scene, pose) it renders, rendered here by the
oracle alone at 72 x 40 with 4 samples and GI -- tiles must mix hits and misses, a good share of the pixels must be lit in
many colours, the camera must be where the pose says it is (below the root, on the centre planes, at a meeting of mirror
masks, inside a solid voxel).  Conditions, not measurements: a pose that fails one is replaced, not excused.  No GPU."""
import os
import sys

import numpy as np
import pytest

import frame_cases as F
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

W, H = F.BASE_SIZE
SPP = 4


def shares(fr):
    hit = (fr.prim["hit"] != 0).mean()
    lit = (fr.accum[..., :3].sum(-1) > 0).mean()
    colours = len(np.unique(fr.accum.reshape(-1, 4), axis=0))
    return hit, lit, colours


def masks_in_one_block(pose, size, block):
    m = F.mirror_masks(pose, *size)
    return max(len(np.unique(m[y:y + block, x:x + block])) for y in range(0, size[1], block) for x in range(0, size[0], block))


@pytest.mark.parametrize("name,depth,k", F.BASE_VIEWS + F.DEEP_VIEWS + F.SHALLOW_VIEWS)
def test_views_mix_hits_and_misses_and_are_lit(name, depth, k):
    import path_schedule as ps
    pose = F.poses(name, depth)[k]
    fr = F.oracle_frame(name, depth, pose, F.light_of(depth), SPP)
    hit, lit, colours = shares(fr)
    print(f"{name} depth {depth} pose {k}: hit share {hit:.3f}, lit share {lit:.3f}, {colours} colours")
    assert 0.2 <= hit <= 0.9
    assert lit >= 0.2
    assert colours >= 50
    # a mixed frame is not enough: 8 x 8 tiles and 4 x 4 quadrants must hold hits next to misses
    h = fr.prim["hit"].reshape(H, W) != 0
    for b in (8, 4):
        blocks = [h[y:y + b, x:x + b] for y in range(0, H, b) for x in range(0, W, b)]
        assert sum(1 for q in blocks if q.any() and not q.all()) >= 5
    cam = F.svo_position(pose, depth)
    nodes = F.scene_nodes(name, depth)
    if k == "a":                                  # general position: camera rays start on the camera's path, below the root
        assert not (cam == 1.5).any()
        if depth >= 3:                            # (a path has whole groups of three rows only: none at depth 2)
            assert ps.camera_path_scale(nodes, depth, cam) < 22
    if k == "b":                                  # on the centre planes: one path per direction-sign variant
        assert (cam[0], cam[2]) == (1.5, 1.5)
        assert max(ps.camera_path_scale(nodes, depth, cam, v) for v in range(8)) < 22
    if k == "c":                                  # four mirror masks in one quadrant, on a camera path that depends on the mask
        assert cam[0] == 1.5 and cam[1] != 1.5 and cam[2] != 1.5
        assert max(ps.camera_path_scale(nodes, depth, cam, v) for v in range(8)) < 22
        assert masks_in_one_block(pose, (W, H), 4) == 4 and masks_in_one_block(pose, (W, H), 8) == 4


def test_small_frames_of_pose_c_still_mix_mirror_masks():
    name, depth, k = F.SIZE_VIEW
    pose = F.poses(name, depth)[k]
    assert masks_in_one_block(pose, (17, 9), 4) == 4      # 17 x 9: four masks in one quadrant
    assert masks_in_one_block(pose, (7, 5), 8) >= 2       # 7 x 5: the one tile is mixed
    for size in F.SMALL_SIZES:
        fr = F.oracle_frame(name, depth, pose, F.light_of(depth), SPP, size=size)
        h = fr.prim["hit"] != 0
        assert h.any() and not h.all() and fr.accum[..., :3].any()


def test_the_object_looks_the_same_at_every_depth():
    """centred at S/2, one generator: the same pixels hit at depths 8, 10 and 11"""
    masks = [F.oracle_frame("bowl", d, F.poses("bowl", d)["a"], F.light_of(d), SPP).prim["hit"] != 0 for d in (8, 10, 11)]
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], masks[2])


@pytest.mark.parametrize("name,depth,k", F.SOLID_VIEWS)
def test_camera_inside_a_solid_voxel(name, depth, k):
    """exempt from the lit share (such a frame is black): every ray hits at t = 0 with an all-zero normal, so the GI
    direction is NaN (test_camera_inside_solid_terminates)"""
    fr = F.oracle_frame(name, depth, F.poses(name, depth)[k], F.light_of(depth), SPP)
    pr = fr.prim
    hit = pr["hit"] != 0
    assert hit.all() and (pr["distance"][hit] == 0).all()
    assert (np.abs(pr["normal"]).sum(1) == 0)[hit].all()
    assert fr.rays > 2 * W * H * SPP                # the shadow and the GI ray are still cast and counted


@pytest.mark.parametrize("which", range(len(F.LIGHTS_ANYWHERE)))
def test_extreme_lights_still_cast_shadow_rays(which):
    """exempt from the lit share; what makes them cases: the frame still mixes hits and misses, and `rays` counts one
    shadow ray per shadow sample of every primary hit, also towards a light at 1e30"""
    name, depth, k = F.LIGHT_VIEW
    pose, light = F.poses(name, depth)[k], F.light_of(depth, which)
    one = F.oracle_frame(name, depth, pose, light, SPP, shadows=1)
    two = F.oracle_frame(name, depth, pose, light, SPP, shadows=2)
    assert 0.2 <= shares(one)[0] <= 0.9
    assert one.hits == two.hits > 0 and two.rays - one.rays == one.hits


def test_shadow_sample_counts_on_the_lattice():
    name, depth, k = F.SHADOW_VIEW
    pose, light = F.poses(name, depth)[k], F.light_of(depth)
    r = {s: F.oracle_frame(name, depth, pose, light, SPP, shadows=s) for s in (0, 1, 2)}
    assert r[0].rays - r[1].rays == 3 * r[1].hits and r[2].rays - r[1].rays == r[1].hits      # 0 = the reference's 4
    assert np.array_equal(r[0].accum, r[2].accum)                                               # the same ray again and again


def test_sharded_view_owns_mixed_rows():
    name, depth, k = F.SHARD_VIEW
    fr = F.oracle_frame(name, depth, F.poses(name, depth)[k], F.light_of(depth), SPP, shard=(8, 1, 3))
    rows = (np.arange(H) // 8) % 3 == 1
    assert (fr.accum[rows, :, 3] == SPP).all() and not fr.accum[~rows].any()
    h = fr.prim["hit"].reshape(H, W)[rows] != 0
    assert h.any() and not h.all() and fr.accum[rows][..., :3].any()


def test_enclosed_poses_are_black_because_the_shadow_ray_has_no_far_limit():
    """docs/NOTEBOOK.md: inside a closed shell nothing is lit, wherever the light is.  Outside, the shell is in the way; inside,
    the shadow ray does not end at the light (raycaster.hpp:150-158 asks for any hit at all) and meets the far wall.  The one
    enclosed view the GPU tests keep is therefore compared on counters and capture, and counts towards no condition above."""
    name, depth, k = F.ENCLOSED_VIEW
    pose = F.poses(name, depth)[k]
    S = float(1 << depth)
    for light in (F.light_of(depth), F.ENCLOSED_LIGHT):
        fr = F.oracle_frame(name, depth, pose, light, SPP)
        hit = fr.prim["hit"] != 0
        assert hit.all() and (fr.prim["distance"] > 0).all() and not fr.accum[..., :3].any()
    o = np.array([[1.5 + 0.2 / S, 1.5 + 36.9 / S, 1.5 + 0.3 / S]], np.float32)            # just inside the wall
    to_light = np.asarray(F.ENCLOSED_LIGHT, np.float32) - o[0]
    reach = float(np.linalg.norm(to_light))
    r = O.cast_rays(F.scene_nodes(name, depth), depth, o, (to_light / reach)[None], 0.0, 0.0)[0]
    assert r["hit"] != 0 and r["distance"] > 1.3 * reach
    # the same view of the OPEN bowl is lit: the cap towards the light is what matters
    fr = F.oracle_frame("bowl", depth, pose, F.light_of(depth), SPP)
    assert (fr.accum[..., :3].sum(-1) > 0).mean() >= 0.2
