"""Times the capsule brush (vrc_stroke_fill_capsules, vrc_stroke_fill_at_hits) next to its yardsticks, on the FastNoise terrain
at 512^3 unless --depth says otherwise, and writes profiles/edit/stroke_timing.json.  Device time by events on the NULL stream,
the median of --pairs rounds A B C A B C after one warm-up round (bench_edit.py's timed_ab); every list is in device memory, so
no staging is timed.  A sample is the call that sets followed by the same call that clears: a brush that finds its voxels
already there skips its atomics, and a set alone would measure that from the second round on.

  thin     one capsule along the whole diagonal, r = 3; the same segment as a sphere of r = 3 at every step of its major axis
           (vrc_volume_fill_spheres); the capsule's bounding box as one box (vrc_volume_fill_boxes)
  strokes  10 000 hits of a crosshair dragged over the terrain, about 3 voxels apart: the strokes between them, r = 3
           (vrc_stroke_fill_at_hits), and a sphere of r = 3 at every hit (vrc_volume_fill_spheres_at_hits)
  fat      one capsule of r = 64 and length 256, and one sphere of r = 64, each also as time per word of the occupancy it holds
           voxels of

    python tools/bench_stroke.py [--depth 9] [--pairs 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_edit import on_device, timed_ab          # noqa: E402  (the timing helpers only; this tool adds no mode there)


def triangle(v, lo, hi):
    span = hi - lo
    w = np.mod(v - lo, 2 * span)
    return lo + np.where(w > span, 2 * span - w, w)


def drag_rays(S, n, step):
    """n nearly parallel rays from outside the volume on the terrain's open side, origins `step` voxels apart along a slanted
    path that turns round at the walls"""
    s = np.arange(n) * float(step)
    x, z = triangle(5.3 + 0.8 * s, 3.0, S - 3.0), triangle(9.7 + 0.6 * s, 3.0, S - 3.0)
    org = np.stack([1.0 + x / S, np.full(n, 0.9), 1.0 + z / S], -1).astype(np.float32)
    d = np.tile(np.array([0.05, 1.0, 0.03]) / np.linalg.norm([0.05, 1.0, 0.03]), (n, 1)).astype(np.float32)
    return org, d


def words_of(volume):
    """the words of the occupancy (2 x 2 x 8 voxels) that hold a solid voxel"""
    vol = volume.download()
    S = vol.shape[0]
    return int((vol.reshape(S // 2, 2, S // 2, 2, S // 8, 8).sum(axis=(1, 3, 5), dtype=np.int64) > 0).sum())


def bench(vrc, depth, pairs):
    S = 1 << depth
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    world = vrc.VoxelVolume.fromScene(scene)
    out = {}

    def both(call):
        return lambda: (call(True), call(False))

    # ---- one thin capsule ----
    e = S - 1
    capsule = on_device(np.array([[0, 0, 0, e, e, e, 3, 0]], np.int32))
    spheres = on_device(np.array([[i, i, i, 3] for i in range(S)], np.int32))
    box = on_device(np.array([[0, 0, 0, S, S, S]], np.uint32))
    a, b, c = timed_ab((both(lambda v: world.fillCapsulesDevice(1, capsule.data_ptr(), v)),
                        both(lambda v: world.fillSpheresDevice(S, spheres.data_ptr(), v)),
                        both(lambda v: world.fillBoxesDevice(1, box.data_ptr(), v))), pairs)
    out["thin"] = {"capsule_set_clear_ms": a, "spheres_on_the_segment_set_clear_ms": b, "bounding_box_set_clear_ms": c, "spheres": S, "radius": 3}
    world.close()

    # ---- hit strokes ----
    world = vrc.VoxelVolume.fromScene(scene)
    n = 10000
    org, d = drag_rays(S, n, 3.0)
    hits = scene.castRays(org, d)
    t_hits = on_device(hits)
    unit = int(((hits["hit"] & 0xff) == 1).sum())
    a, b = timed_ab((both(lambda v: world.strokeAtHitsDevice(n, t_hits.data_ptr(), 3, v)),
                     both(lambda v: world.fillSpheresAtHitsDevice(n, t_hits.data_ptr(), 3, v))), pairs)
    out["strokes"] = {"stroke_at_hits_dig_build_ms": a, "spheres_at_hits_dig_build_ms": b, "records": n, "unit_voxel_hits": unit, "radius": 3}
    world.close()

    # ---- one fat capsule ----
    m = S // 2
    fat = np.array([[m - 128, m, m, m + 128, m, m, 64, 0]], np.int32)
    ball = np.array([[m, m, m, 64]], np.int32)
    t_fat, t_ball = on_device(fat), on_device(ball)
    empty = vrc.VoxelVolume(depth)
    empty.fillCapsules(fat, True)
    fat_words = words_of(empty)
    empty.fillCapsules(fat, False)
    empty.fillSpheres(ball, True)
    ball_words = words_of(empty)
    empty.fillSpheres(ball, False)
    a, b = timed_ab((both(lambda v: empty.fillCapsulesDevice(1, t_fat.data_ptr(), v)), both(lambda v: empty.fillSpheresDevice(1, t_ball.data_ptr(), v))), pairs)
    out["fat"] = {"capsule_set_clear_ms": a, "sphere_set_clear_ms": b, "capsule_words": fat_words, "sphere_words": ball_words,
                  "capsule_ns_per_word": round(a["median"] * 1e6 / (2 * fat_words), 3), "sphere_ns_per_word": round(b["median"] * 1e6 / (2 * ball_words), 3),
                  "radius": 64, "length": 256}
    empty.close()
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    import cpuvoxelraycaster_amd as vrc
    if not torch.cuda.is_available():
        raise SystemExit("bench_stroke.py needs a GPU (the library has no CPU fallback)")
    out = {"bench": "stroke", "device": torch.cuda.get_device_name(0), "depths": {str(args.depth): bench(vrc, args.depth, max(1, args.pairs))}}
    print(json.dumps(out))
    with open(os.path.join(ROOT, "profiles", "edit", "stroke_timing.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
