#!/usr/bin/env python3
"""Generate tests/golden/swarm_frames_d7_162x91.npz with the REAL swarm thread pool of the reference (lib/swarm/swarm.hpp
compiled where it lies into oracle/_ref/libref_swarm.so, oracle/Makefile) driving the oracle's per-area frame job: the
accumulators and the ray / loop-iteration counts after six frame-samples of the depth-7 terrain at 162 x 91, the case of
tests/test_oracle_pins.py::test_frame_on_the_references_own_swarm_pool.  Runs only where the reference is mounted.  The
fixture is data: what the reference's pool produced."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden", "swarm_frames_d7_162x91.npz")

DEPTH, W, H, FRAMES = 7, 162, 91, 6


def swarm_frames(O, heights, textures):
    """six frame-samples on the reference's swrm::Swarm(16): (accumulators, rays, loop iterations)"""
    import cpuvoxelraycaster_amd as vrc
    nodes = O.compile_terrain(DEPTH, heights)
    top, side = textures
    cam = O.make_camera(vrc.reference_camera_position(DEPTH), O.make_rotation(0.0, -0.5))
    light = vrc.reference_light(DEPTH)
    sw = O.RefSwarm(16)
    acc, rays, steps = None, 0, 0
    for s in range(FRAMES):
        p = O.make_params(W, H, light, use_gi=1, use_samples=1, shadow_samples=1, frame_index=s)
        _, acc, st = sw.render_frame(nodes, DEPTH, top, side, cam, p, accum=acc)
        rays, steps = rays + st.rays, steps + st.sum_complexity
    sw.close()
    return acc, rays, steps


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libvrc_oracle.so", "ref"], stdout=subprocess.DEVNULL)
    import oracle_lib as O
    if not O.RefSwarm.available():
        sys.exit("oracle/_ref/libref_swarm.so was not built (the reference is not mounted)")
    acc, rays, steps = swarm_frames(O, O.load_terrain_heights(), O.load_textures())
    assert acc.max() < 1 << 16
    np.savez_compressed(GOLD, accum=acc.astype(np.uint16), rays=np.int64(rays), sum_complexity=np.int64(steps))
    print(GOLD, acc.shape, rays, steps)


if __name__ == "__main__":
    main()
