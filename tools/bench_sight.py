"""Times vrc_sight_segments and vrc_sight_field next to their yardsticks at 512^3 unless --depth says otherwise, on the FastNoise
terrain with the Euclidean field to the solid, and writes profiles/edit/sight_timing.json.  Device time by events on the NULL
stream, the median of --pairs rounds A B C ... A B C ... after one warm-up round (bench_edit.py's timed_ab); segments and
records are in device memory, so no staging is timed.

  segments  2^20 (--segments) segments between random air voxels, THIN:
            stride_r0 / plain_r0   lo = 1: a thin ray, striding and with VRC_SIGHT_PLAIN
            stride_r2 / plain_r2   lo = 5: a ball of radius 2
            distance_at            vrc_distance_at at exactly as many random voxels as the plain walk of r0 loads at least (per
                                   segment the dominant-axis distance from a to the record's `at`, plus one): the floor of that
                                   many scattered loads, which the plain walk is held against; the stride makes fewer
            cast_rays              vrc_cast_rays on the committed scene, the same endpoints as float rays of length |b - a|
  field     vrc_sight_field from an eye above the terrain with radius 64 and 128, next to vrc_volume_distance_field itself

    python tools/bench_sight.py [--depth 9] [--pairs 5] [--segments 1048576]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_edit import timed_ab          # noqa: E402  (the helpers only; this tool adds no mode there)


def air_segments(field, S, n, seed):
    """(n, 6) int32 between random voxels with D > 0"""
    rng = np.random.default_rng(seed)
    got = np.zeros((0, 3), np.uint32)
    while len(got) < 2 * n:
        xyz = rng.integers(0, S, (2 * n, 3)).astype(np.uint32)
        got = np.concatenate([got, xyz[field.at(xyz) > 0]])
    return got[:2 * n].reshape(n, 6).astype(np.int32)


def bench(vrc, depth, pairs, n):
    import torch
    capi = vrc.capi
    S = 1 << depth
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    world = vrc.VoxelVolume.fromScene(scene)
    field = world.distanceField()
    segments = air_segments(field, S, n, depth)
    d_segments = torch.from_numpy(segments).cuda()
    d_records = torch.zeros(n * 8, dtype=torch.int32, device="cuda")

    def sight(lo, plain):
        field.sightDevice(n, d_segments.data_ptr(), d_records.data_ptr(), lo, capi.VRC_DISTANCE_NONE, False, plain)

    def records(lo, plain):
        sight(lo, plain)
        return d_records.cpu().numpy().view(capi.SIGHT_DTYPE).copy()

    plain_r0 = records(1, True)
    same = {"r0": records(1, False).tobytes() == plain_r0.tobytes(), "r2": records(5, False).tobytes() == records(5, True).tobytes()}
    loads = int((np.abs(plain_r0["at"].astype(np.int64) - segments[:, :3]).max(axis=1) + 1).sum())
    points = loads                                             # the same number of loads: 12 bytes of coordinates and 4 of values each
    d_xyz = torch.randint(0, S, (points, 3), dtype=torch.int32, device="cuda")
    d_values = torch.zeros(points, dtype=torch.int32, device="cuda")
    # the same endpoints as float rays in the scene's cube [1, 2)^3: t = 1 is the centre of b
    org = (1.0 + (segments[:, :3] + 0.5) / S).astype(np.float32)
    dir_ = ((segments[:, 3:] - segments[:, :3]) / S).astype(np.float32)
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(dir_).cuda()
    d_hits = torch.zeros(n * 12, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    names = ["stride_r0_ms", "plain_r0_ms", "stride_r2_ms", "plain_r2_ms", "distance_at_ms", "cast_rays_ms"]
    fns = [lambda: sight(1, False), lambda: sight(1, True), lambda: sight(5, False), lambda: sight(5, True),
           lambda: field.atDevice(points, d_xyz.data_ptr(), d_values.data_ptr()), lambda: scene.castRaysDevice(n, d_org.data_ptr(), d_dir.data_ptr(), d_hits.data_ptr())]
    out = {"segments": n, "blocked_r0": int((plain_r0["status"] == capi.VRC_SIGHT_BLOCKED).sum()), "loads_at_least": loads, "distance_at_points": points,
           "stride_same_bytes_as_plain": same}
    out.update(dict(zip(names, timed_ab(fns, pairs))))
    for r in ("r0", "r2"):
        out["stride_over_plain_" + r] = round(out["stride_%s_ms" % r]["median"] / out["plain_%s_ms" % r]["median"], 3)
    out["plain_r0_over_distance_at"] = round(out["plain_r0_ms"]["median"] / out["distance_at_ms"]["median"], 3)
    out["stride_r0_over_cast_rays"] = round(out["stride_r0_ms"]["median"] / out["cast_rays_ms"]["median"], 3)

    eye = (S // 2, S * 200 // 512, S // 2)                     # above the terrain, which is solid from y = S/2 + 1 on
    radii = (S // 8, S // 4)
    names = ["sight_field_r%d_ms" % r for r in radii] + ["sight_field_r%d_plain_ms" % r for r in radii] + ["distance_field_ms"]
    fns = [lambda r=r: field.visibleFrom(eye, r) for r in radii] + [lambda r=r: field.visibleFrom(eye, r, plain=True) for r in radii] + [lambda: world.distanceField()]
    sight_out = {"eye": eye, "eye_d2": int(field.at(np.array([eye], np.uint32))[0])}
    sight_out.update(dict(zip(names, timed_ab(fns, pairs))))
    for r in radii:
        seen = field.visibleFrom(eye, r)
        sight_out["visible_r%d" % r] = int(seen.stats.visible)
        sight_out["sight_field_r%d_over_distance_field" % r] = round(sight_out["sight_field_r%d_ms" % r]["median"] / sight_out["distance_field_ms"]["median"], 3)
        seen.close()
    for handle in (field, world, scene):
        handle.close()
    return {"size": S, "pairs": pairs, "segments": out, "field": sight_out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--segments", type=int, default=1 << 20)
    args = ap.parse_args()
    if not 6 <= args.depth <= 9:
        raise SystemExit("bench_sight.py: --depth is 6 .. 9")
    import __graft_entry__ as g
    g.build()
    import torch
    import cpuvoxelraycaster_amd as vrc
    if not torch.cuda.is_available():
        raise SystemExit("bench_sight.py needs a GPU (the library has no CPU fallback)")
    out = {"bench": "sight", "device": torch.cuda.get_device_name(0),
           "depths": {str(args.depth): bench(vrc, args.depth, max(1, args.pairs), max(1, args.segments))}}
    print(json.dumps(out))
    with open(os.path.join(ROOT, "profiles", "edit", "sight_timing.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
