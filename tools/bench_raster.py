"""Times the surface voxelisation (vrc_raster_mesh, both modes) next to a yardstick from the same run, at 512^3 unless
--depth says otherwise, and writes profiles/edit/raster_timing.json.  Device time by events on the NULL stream, the median of
--pairs rounds A B C A B C after one warm-up round (bench_edit.py's timed_ab); every list is in device memory, so no staging is
timed.  A sample is the call that sets followed by the same call that clears -- a call that finds its voxels already there skips
its atomics -- and for vrc_volume_xor_mesh the call twice, which restores the volume.  Everything goes into an empty volume.

  terrain   the closed merged-rectangle surface mesh of the FastNoise terrain (rectTriangles), TOUCHED and THIN, next to
            vrc_volume_xor_mesh of the same triangles
  corner    the one triangle (0,0,0) (S,S,0) (S,0,S) that spans the volume corner to corner, TOUCHED and THIN, next to
            vrc_volume_fill_boxes of its bounding box, the whole volume
  small     100 000 unit-face triangles, the first of the face mesh (surfaceTriangles) of a seeded 128^3 noise field, TOUCHED and
            THIN, next to vrc_volume_xor_mesh of the same

Each case runs in a process of its own under a time limit, and the first one that fails ends the run.

    python tools/bench_raster.py [--depth 9] [--pairs 5]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = ("terrain", "corner", "small")
CASE_SECONDS = 240


def ratio(a, b):
    return round(a["median"] / b["median"], 2) if b["median"] > 0 else None


def mesh_case(vrc, target, tris, pairs, label):
    """TOUCHED, THIN and xor_mesh of the same triangles into `target`"""
    from bench_edit import on_device, timed_ab
    n = len(tris)
    t = on_device(np.ascontiguousarray(tris, np.int32))
    T, H = vrc.capi.VRC_RASTER_TOUCHED, vrc.capi.VRC_RASTER_THIN
    counts = {}
    for name, mode in (("touched", T), ("thin", H)):
        target.rasterMesh((n, t.data_ptr()), mode, True, device=True)
        counts[name + "_voxels"] = target.solidCount()
        target.rasterMesh((n, t.data_ptr()), mode, False, device=True)
    assert target.solidCount() == 0
    a, b, c = timed_ab((lambda: [target.rasterMesh((n, t.data_ptr()), T, v, device=True) for v in (True, False)],
                        lambda: [target.rasterMesh((n, t.data_ptr()), H, v, device=True) for v in (True, False)],
                        lambda: [target.xorMesh((n, t.data_ptr()), device=True) for _ in (0, 1)]), pairs)
    assert target.solidCount() == 0
    out = {"triangles": n, "touched_set_clear_ms": a, "thin_set_clear_ms": b, label: c, "touched_over_yardstick": ratio(a, c),
           "thin_over_yardstick": ratio(b, c)}
    out.update(counts)
    return out


def run_case(vrc, case, depth, pairs):
    from bench_edit import on_device, timed_ab
    S = 1 << depth
    target = vrc.VoxelVolume(depth)
    if case == "terrain":
        scene = vrc.LSVO.fromFastNoiseTerrain(depth)
        world = vrc.VoxelVolume.fromScene(scene)
        tris = world.rectTriangles(closed=True)
        world.close()
        scene.close()
        out = mesh_case(vrc, target, tris, pairs, "xor_mesh_twice_ms")
    elif case == "small":
        field = vrc.VoxelVolume(7)
        field.setVoxels(np.argwhere(np.random.default_rng(128).random((128, 128, 128)) < 0.5))
        tris = field.surfaceTriangles(closed=True, capacity=50000)
        field.close()
        out = mesh_case(vrc, target, tris, pairs, "xor_mesh_twice_ms")
    else:
        far = 64 * S
        t = on_device(np.array([[0, 0, 0, far, far, 0, far, 0, far]], np.int32))
        box = on_device(np.array([[0, 0, 0, S, S, S]], np.uint32))
        T, H = vrc.capi.VRC_RASTER_TOUCHED, vrc.capi.VRC_RASTER_THIN
        counts = {}
        for name, mode in (("touched", T), ("thin", H)):
            target.rasterMesh((1, t.data_ptr()), mode, True, device=True)
            counts[name + "_voxels"] = target.solidCount()
            target.rasterMesh((1, t.data_ptr()), mode, False, device=True)
        a, b, c = timed_ab((lambda: [target.rasterMesh((1, t.data_ptr()), T, v, device=True) for v in (True, False)],
                            lambda: [target.rasterMesh((1, t.data_ptr()), H, v, device=True) for v in (True, False)],
                            lambda: [target.fillBoxesDevice(1, box.data_ptr(), v) for v in (True, False)]), pairs)
        assert target.solidCount() == 0
        out = {"triangles": 1, "touched_set_clear_ms": a, "thin_set_clear_ms": b, "bounding_box_set_clear_ms": c,
               "touched_over_yardstick": ratio(a, c), "thin_over_yardstick": ratio(b, c)}
        out.update(counts)
    target.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--case", choices=CASES, help="run this case alone and print its result (what the tool starts for each case)")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    if args.case:
        import torch
        import cpuvoxelraycaster_amd as vrc
        if not torch.cuda.is_available():
            raise SystemExit("bench_raster.py needs a GPU (the library has no CPU fallback)")
        print(json.dumps({"device": torch.cuda.get_device_name(0), "result": run_case(vrc, args.case, args.depth, max(1, args.pairs))}))
        return
    out = {"bench": "raster", "device": None, "depths": {str(args.depth): {}}}
    for case in CASES:                       # a process each, so that a case that faults or hangs ends the run and starts nothing more
        cmd = [sys.executable, os.path.abspath(__file__), "--depth", str(args.depth), "--pairs", str(args.pairs), "--case", case]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=CASE_SECONDS)
        if done.returncode != 0:
            raise SystemExit("bench_raster.py: case %s ended with status %d\n%s" % (case, done.returncode, (done.stdout + done.stderr)[-2000:]))
        one = json.loads(done.stdout.strip().splitlines()[-1])
        out["device"] = one["device"]
        out["depths"][str(args.depth)][case] = one["result"]
    print(json.dumps(out))
    with open(os.path.join(ROOT, "profiles", "edit", "raster_timing.json"), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
