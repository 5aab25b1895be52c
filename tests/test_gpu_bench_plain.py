"""The plain benchmark line (`bench.py --gpus 1 --steps K --warmup W`): exactly K timed frames in one block, none of the --full
checks or extras in the line, and --dump-outputs writes the frame of the last timed step -- which must be the oracle's frame
W + K - 1 of the same workload, bit for bit (config c2: 256^3 terrain, 1280x720, primary + shadow ray, cheap for the oracle), at
N = 1 and, with two ranks sharing the GPU, for the gathered frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def oracle_c2_frame(vrc, textures, frame):
    """frame `frame` of config c2 (1 spp, no GI) as the oracle renders it"""
    depth, W, H = 8, 1280, 720
    top, side = textures
    nodes = O.compile_terrain(depth, O.terrain_heights(1 << depth))
    cam = vrc.reference_camera(depth, pitch=-0.5)
    ocam = O.make_camera(tuple(cam.position), tuple(cam.rot), cam.fov, cam.aperture, cam.focal_length)
    p = O.make_params(W, H, vrc.reference_light(depth), use_gi=0, use_samples=1, shadow_samples=1, frame_index=frame)
    _, acc, _, _ = O.render_frame(nodes, depth, top, side, ocam, p, threads=min(16, os.cpu_count() or 4))
    return O.samples_to_image(acc).astype(np.float32)


def run_plain(world, steps, warmup, out_dir, extra_env=None, extra_args=()):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(extra_env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", str(steps), "--warmup", str(warmup),
                          "--config", "c2", "--dump-outputs", str(out_dir)] + list(extra_args), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["n_gpus"] == world and d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0
    assert d["extra"]["ms_per_step_blocks"]["blocks"] == 1
    assert abs(d["value"] - d["config"]["rays_per_frame"] / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
    assert "cpu_baseline" not in d and d["config"]["frame_equals_oracle"] is None
    assert set(d["extra"]) == {"ms_per_step_blocks"}
    img = np.load(out_dir / "image.npy")
    assert img.dtype == np.float32 and img.shape == (720, 1280, 4)
    return d, img


def test_plain_line_times_k_steps_and_dumps_the_last_frame(built, tmp_path, textures):
    import cpuvoxelraycaster_amd as vrc
    steps, warmup = 4, 2
    d, img = run_plain(1, steps, warmup, tmp_path / "outputs")
    assert d["config"]["rays_per_frame"] > 0
    assert np.array_equal(img, oracle_c2_frame(vrc, textures, warmup + steps - 1))


@pytest.mark.parametrize("gather", ["root", "peer"])
def test_plain_line_at_two_ranks_dumps_the_gathered_frame(built, tmp_path, textures, gather):
    """N = 2 ranks sharing the box's GPU (gloo rehearsal for 'root'; real hipIpc peer writes for 'peer'): the frame rank 0
    dumps is the composed frame of the last timed step, equal to the oracle's"""
    import cpuvoxelraycaster_amd as vrc
    steps, warmup = 5, 2
    d, img = run_plain(2, steps, warmup, tmp_path / "outputs", {"VRC_DIST_BACKEND": "gloo"}, ["--gather", gather])
    assert d["config"]["ranks_in_process_group"] == 2 and "exchange_forms" not in d["extra"]
    assert d["config"]["gathered_frame_equals_unsharded"] is None
    assert np.array_equal(img, oracle_c2_frame(vrc, textures, warmup + steps - 1))
