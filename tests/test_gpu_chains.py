"""vrc_cast_ray_chains against its stated contract (include/vrc.h): out_b[i] equals vrc_cast_rays of ray B alone bit for bit,
for the caller's origins and directions WHATEVER THEY ARE -- next to A's hit as the frame kernels put them, anywhere in the
cube, outside it, on its planes, non-finite, or A over again -- on shallow trees, the terrain and the deepest tree the
library takes, with misses of A among the hits.  The oracle walks every ray from the root (lsvo.hpp:60-72); the operator
starts B below the root on the path A's walk left (csrc/vrc_device.h: start_scale_next_to[_lod], ray_start_below).
tests/tools/fuzz_gpu.py --chains runs the same generator for any seed and ray count."""
import numpy as np
import pytest

import edge_cases as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

SCENES = ["terrain8", "volume2", "volume3", "volume5", "sparse11"]
N_RAYS = {"terrain8": 200000, "volume2": 20000, "volume3": 20000, "volume5": 50000, "sparse11": 50000}


def chain_scene(name, heights):
    """(nodes, depth, light, points to aim ray A at or None, camera position in [1, 2)^3)"""
    import cpuvoxelraycaster_amd as vrc
    f = np.float32
    if name == "terrain8":
        cam = (np.asarray(vrc.reference_camera(8).position, f) * (f(1.0) / f(256.0)) + f(1.0)).astype(f)    # main.cpp:149
        return vrc.build_terrain_lsvo(heights, 8), 8, np.asarray(vrc.reference_light(8), f), None, cam
    if name == "sparse11":                                   # the scene of test_gpu_cast.test_maximum_depth_scene
        depth, S = 11, 2048
        rng = np.random.default_rng(42)
        vox = rng.integers(0, S, (300, 3))
        vox = np.concatenate([vox, [[0, 0, 0], [S - 1, S - 1, S - 1], [1024, 1024, 1024], [1023, 1023, 1023]]])
        # the walk sees the scene point-reflected through the cube centre (lsvo.hpp:79): voxel v appears at S - 1 - v
        targets = ((S - 1 - vox + 0.5) / S + 1.0).astype(f)
        return O.compile_voxels(depth, vox), depth, np.asarray([1.3, 1.9, 1.6], f), targets, np.asarray([1.5, 1.39, 1.5], f)
    depth = int(name[len("volume"):])
    rng = np.random.default_rng(100 + depth)
    vol = E.carved_volume(depth, rng)
    # the camera anywhere in the cube (on the centre planes no ray next to it can start below the root)
    return (O.compile_voxels(depth, np.argwhere(vol).astype(np.int64)), depth, np.asarray([1.3, 1.9, 1.6], f), None,
            rng.uniform(1.05, 1.95, 3).astype(f))


@pytest.fixture(scope="module")
def scenes(built, heights, textures):
    import cpuvoxelraycaster_amd as vrc
    out = {}
    for name in SCENES:
        nodes, depth, light, targets, cam = chain_scene(name, heights)
        out[name] = (nodes, depth, light, targets, cam, vrc.LSVO(nodes, depth, textures=textures))
    return out


@pytest.mark.parametrize("kind", E.CHAIN_KINDS)
@pytest.mark.parametrize("scene", SCENES)
def test_chains_equal_two_casts_of_the_oracle(scenes, scene, kind):
    nodes, depth, light, targets, cam, svo = scenes[scene]
    rng = np.random.default_rng(SCENES.index(scene) * 16 + E.CHAIN_KINDS.index(kind))
    org_a, dir_a = E.chain_rays_a(depth, N_RAYS[scene], rng, targets, cam)
    cast_oracle = lambda o, d, coef: O.cast_rays(nodes, depth, o, d, coef, 0.0, threads=8)
    stats = E.check_chains(E.gpu_chain_caster(svo), cast_oracle, depth, kind, org_a, dir_a, light, rng)
    print(f"chains {scene} {kind}: {stats}")
    assert 0.1 * stats["n"] < stats["hits_a"] < 0.95 * stats["n"]            # hits and misses of A side by side
    if kind == "non_finite":
        assert stats["non_finite_b"] > 0.5 * stats["n"]
