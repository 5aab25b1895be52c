"""Times the calls between depths (vrc_levels_counts, vrc_levels_reduce, vrc_levels_expand) next to their yardsticks at 512^3
unless --depth says otherwise, and writes profiles/edit/levels_timing.json.  Device time by events on the NULL stream around
--calls calls in a row, the median of --pairs rounds A B C ... A B C ... after one warm-up round (bench_edit.py's timed_ab);
the counts go to device memory, so no staging is timed.

  terrain  the FastNoise terrain
  random   a seeded random field of density 0.5 (vrc_cells_fill_random)
           on each: the counts at k = 1, 3, 5 and k = depth, the reduction "any" to depth - 1, depth - 3 and 2, and the expansion of
           the depth - 1 reduction back to the depth; in the same rounds vrc_volume_clone of the source (the same bytes read, no
           arithmetic), vrc_volume_solid_count, and for the expansion vrc_volume_stamp_affine with the exact map
           m = diag(65536 >> 1), t = 0

    python tools/bench_levels.py [--depth 9] [--pairs 5] [--calls 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_edit import timed_ab          # noqa: E402  (the helpers only; this tool adds no mode there)


def field_case(vrc, src, pairs, calls):
    import torch
    depth = src.depth
    ks = sorted({1, 3, 5, depth})
    to = sorted({depth - 1, depth - 3, 2}, reverse=True)
    counts = {k: torch.empty(8 ** (depth - k), dtype=torch.int32, device="cuda") for k in ks}
    coarse = {d: vrc.VoxelVolume(d) for d in to}
    fine = vrc.VoxelVolume(depth)
    half = vrc.make_affine([32768, 0, 0, 0, 32768, 0, 0, 0, 32768], [0, 0, 0])
    src.reduceInto(coarse[depth - 1], *vrc.count_range("any", 1))
    torch.cuda.synchronize()
    names = ["clone_ms", "solid_count_ms"] + ["counts_k%d_ms" % k for k in ks] + ["reduce_any_to_%d_ms" % d for d in to] + ["expand_ms", "stamp_affine_ms"]
    fns = [lambda: src.clone(), lambda: src.solidCount()]
    fns += [lambda k=k: src.cellCountsDevice(k, counts[k].data_ptr()) for k in ks]
    fns += [lambda d=d: src.reduceInto(coarse[d], *vrc.count_range("any", depth - d)) and None for d in to]
    fns += [lambda: coarse[depth - 1].expandInto(fine) and None, lambda: fine.stampAffine(coarse[depth - 1], half)]
    out = {"solid": src.solidCount(), "source_bytes": 8 ** (depth - 1)}
    out.update(dict(zip(names, timed_ab(fns, pairs, calls))))
    for k in ks:
        assert int(counts[k].sum(dtype=torch.int64)) == out["solid"], k
    for v in list(coarse.values()) + [fine]:
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
        raise SystemExit("bench_levels.py: --depth is 6 .. 10")
    import __graft_entry__ as g
    g.build()
    import torch
    import cpuvoxelraycaster_amd as vrc
    if not torch.cuda.is_available():
        raise SystemExit("bench_levels.py needs a GPU (the library has no CPU fallback)")
    out = {"bench": "levels", "device": torch.cuda.get_device_name(0),
           "depths": {str(args.depth): bench(vrc, args.depth, max(1, args.pairs), max(1, args.calls))}}
    print(json.dumps(out))
    with open(os.path.join(ROOT, "profiles", "edit", "levels_timing.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
