#!/usr/bin/env python3
"""Times the editable volume (vrc_volume_*) on the device, one JSON line.

For the 256^3, 512^3 and 1024^3 FastNoise terrain:
  from_scene_ms    wall time of vrc_volume_from_scene (allocation + rasterisation kernel, synchronous), median of 3
  set_voxels_ms    device time (events on the stream) of one vrc_volume_set_voxels batch of 1 / 1 000 / 10^6 random
                   voxels read from device memory, median of 5
  fill_box_64_ms   device time of one 64^3 box (vrc_volume_fill_boxes), median of 5
  commit_ms / build_volume_ms
                   vrc_volume_commit's build_ms against vrc_scene_build_volume's build_ms for the SAME occupancy in the
                   same process, alternating A B A B, `--pairs` pairs after one warm-up pair: medians, the baseline's
                   own min / max over its repetitions, and whether the commit's median lies within that spread
                   (commit_within_baseline_spread: commit median <= baseline max).
No threshold is applied; the numbers are reported."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_ms(fn, repeats=5):
    import torch
    out = []
    for i in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:                                        # the first run warms up
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def bench_depth(vrc, depth, pairs):
    import torch
    S = 1 << depth
    rng = np.random.default_rng(depth)
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    res = {"size": S, "nodes": scene.n_nodes}
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        volume = vrc.VoxelVolume.fromScene(scene)
        walls.append((time.perf_counter() - t0) * 1e3)
        if _ < 2:
            volume.close()
    res["from_scene_ms"] = round(statistics.median(walls), 4)
    scene.close()
    res["solid_voxels"] = volume.solidCount()

    # commit against the one-shot builder on the same occupancy (the untouched terrain), A B A B
    dense = volume.download()
    commit, build = [], []
    for i in range(pairs + 1):
        a = volume.commit()
        b = vrc.LSVO.fromVolume(dense, depth)
        assert a.n_nodes == b.n_nodes
        if i:
            commit.append(a.build_ms)
            build.append(b.build_ms)
        a.close()
        b.close()
    res["commit_ms"] = {"median": round(statistics.median(commit), 4), "min": round(min(commit), 4), "max": round(max(commit), 4)}
    res["build_volume_ms"] = {"median": round(statistics.median(build), 4), "min": round(min(build), 4), "max": round(max(build), 4)}
    res["commit_within_baseline_spread"] = bool(statistics.median(commit) <= max(build))
    res["pairs"] = pairs

    # edits: device memory, the NULL stream (where torch's events are recorded)
    res["set_voxels_ms"] = {}
    for n in (1, 1000, 1000000):
        xyz = torch.from_numpy(rng.integers(0, S, (n, 3)).astype(np.int32)).cuda()
        flip = [False]

        def one():
            flip[0] = not flip[0]
            volume.setVoxelsDevice(n, xyz.data_ptr(), flip[0], None)
        device_ms(one, 2)
        res["set_voxels_ms"][str(n)] = round(device_ms(one, 5), 5)
    lo = S // 2 - 32
    box = torch.tensor([lo, lo, lo, lo + 64, lo + 64, lo + 64], dtype=torch.int32).cuda()
    res["fill_box_64_ms"] = round(device_ms(lambda: volume.fillBoxesDevice(1, box.data_ptr(), True, None)), 5)
    volume.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depths", type=int, nargs="+", default=[8, 9, 10])
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    import cpuvoxelraycaster_amd as vrc
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit.py needs a GPU (the library has no CPU fallback)")
    out = {"bench": "edit", "device": torch.cuda.get_device_name(0), "depths": {}}
    for d in args.depths:
        out["depths"][str(d)] = bench_depth(vrc, d, max(1, args.pairs))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
