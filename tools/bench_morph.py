"""Times vrc_morph_apply next to its yardsticks at 512^3 unless --depth says otherwise, and writes
profiles/edit/morph_timing.json.  Device time by events on the NULL stream around --calls calls in a row, the median of --pairs
rounds A B C ... A B C ... after one warm-up round (bench_edit.py's timed_ab); every list is in device memory, so no staging is
timed.  All forms are DILATE of the solid voxels into a second volume, REPLACE.

  terrain  the FastNoise terrain
  random   a seeded random field of density 0.5 (vrc_cells_fill_random)
           on each, in the same rounds:
           cube3 / cross        the 3 x 3 x 3 cube and the cross  next to  vrc_cells_step with 26 / 6 neighbours giving the same bits
           ball_r2 / r4 / r8    element_ball(r)                   next to  vrc_volume_distance_field + vrc_distance_select, today's
                                                                           dilate(r), with the device bytes each holds
           box9 / box9_lines    the 9 x 9 x 9 box as one call     next to  the same box as three line calls
           line33_x / _y / _z   the full-reach line of 33 voxels on each axis

    python tools/bench_morph.py [--depth 9] [--pairs 5] [--calls 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_edit import timed_ab          # noqa: E402  (the helpers only; this tool adds no mode there)

BLOCK_BYTES = 13312                      # the prepared element (include/vrc.h)


def field_case(vrc, src, pairs, calls):
    import torch
    capi = vrc.capi
    depth = src.depth
    dst, other, third = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
    elements = {"cube3": vrc.element_box(3, 3, 3), "cross": vrc.element_cross(), "box9": vrc.element_box(9, 9, 9)}
    elements.update({"ball_r%d" % r: vrc.element_ball(r) for r in (2, 4, 8)})
    elements.update({"line33_" + "xyz"[a]: vrc.element_line(a, -16, 16) for a in range(3)})
    elements.update({"line9_" + "xyz"[a]: vrc.element_line(a, -4, 4) for a in range(3)})
    lists = {k: torch.from_numpy(e).cuda() for k, e in elements.items()}
    torch.cuda.synchronize()

    def morph(name, a=src, b=dst):
        a.morphDevice(b, capi.VRC_MORPH_DILATE, len(elements[name]), lists[name].data_ptr())

    def by_distance(r):
        field = src.distanceField()
        field.select(0, r * r, other, capi.VRC_COPY_REPLACE)
        field.close()

    def three_lines():
        morph("line9_x", src, other)
        morph("line9_y", other, third)
        morph("line9_z", third, other)

    grow26, stay26, grow6, stay6 = vrc.count_mask(range(1, 27)), vrc.count_mask(range(0, 27)), vrc.count_mask(range(1, 7)), vrc.count_mask(range(0, 7))
    names = ["cube3_ms", "cells_step_26_ms", "cross_ms", "cells_step_6_ms", "box9_ms", "box9_lines_ms"] + ["line33_%s_ms" % a for a in "xyz"]
    fns = [lambda: morph("cube3"), lambda: src.cellStepDevice(other, grow26, stay26, None, 26), lambda: morph("cross"), lambda: src.cellStepDevice(other, grow6, stay6, None, 6),
           lambda: morph("box9"), three_lines] + [lambda a=a: morph("line33_" + a) for a in "xyz"]
    for r in (2, 4, 8):
        names += ["ball_r%d_ms" % r, "distance_dilate_r%d_ms" % r]
        fns += [lambda r=r: morph("ball_r%d" % r), lambda r=r: by_distance(r)]
    out = {"solid": src.solidCount(), "source_bytes": 8 ** depth // 8, "element_bytes": BLOCK_BYTES, "distance_field_bytes": 4 * 8 ** depth,
           "offsets": {k: len(e) for k, e in elements.items()}}
    out.update(dict(zip(names, timed_ab(fns, pairs, calls))))
    # the yardsticks give the same bits
    same = {}
    for name, (grow, stay, neighbours) in {"cube3": (grow26, stay26, 26), "cross": (grow6, stay6, 6)}.items():
        morph(name)
        src.cellStepDevice(other, grow, stay, None, neighbours)
        same[name] = bool(dst.diff(other).stats.words == 0)
    morph("box9")
    three_lines()
    same["box9_lines"] = bool(dst.diff(other).stats.words == 0)
    for r in (2, 4, 8):
        morph("ball_r%d" % r)
        by_distance(r)
        other.copyRegion(src, (0, 0, 0), (1 << depth,) * 3, (0, 0, 0), capi.VRC_COPY_OR)
        same["ball_r%d" % r] = bool(dst.diff(other).stats.words == 0)
    out["same_bits_as_yardstick"] = same
    for k in ("cube3", "cross"):
        out[k + "_over_cells_step"] = round(out[k + "_ms"]["median"] / out["cells_step_%d_ms" % (26 if k == "cube3" else 6)]["median"], 3)
    out["box9_over_lines"] = round(out["box9_ms"]["median"] / out["box9_lines_ms"]["median"], 3)
    for r in (2, 4, 8):
        out["ball_r%d_over_distance" % r] = round(out["ball_r%d_ms" % r]["median"] / out["distance_dilate_r%d_ms" % r]["median"], 3)
    for v in (dst, other, third):
        v.close()
    return out


def bench(vrc, depth, pairs, calls):
    out = {"size": 1 << depth, "pairs": pairs, "calls": calls}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    world = vrc.VoxelVolume.fromScene(scene)
    out["terrain"] = field_case(vrc, world, pairs, calls)
    world.close()
    scene.close()
    noise = vrc.VoxelVolume(depth)
    noise.fillRandom(depth, 0.5)
    out["random"] = field_case(vrc, noise, pairs, calls)
    noise.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if not 6 <= args.depth <= 10:
        raise SystemExit("bench_morph.py: --depth is 6 .. 10")
    import __graft_entry__ as g
    g.build()
    import torch
    import cpuvoxelraycaster_amd as vrc
    if not torch.cuda.is_available():
        raise SystemExit("bench_morph.py needs a GPU (the library has no CPU fallback)")
    out = {"bench": "morph", "device": torch.cuda.get_device_name(0),
           "depths": {str(args.depth): bench(vrc, args.depth, max(1, args.pairs), max(1, args.calls))}}
    print(json.dumps(out))
    with open(os.path.join(ROOT, "profiles", "edit", "morph_timing.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
