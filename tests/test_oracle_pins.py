"""Pins the CPU oracle against what is known about the unmodified reference:
the statistics SURVEY.md App. B / section 6 measured by running it (node counts,
first nodes, level histogram, per-pose hit counts, loop-iteration statistics,
normal-axis split, one sample hit).  The reference holds no tests or golden
vectors of its own."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nodes9(heights):
    return O.compile_terrain(9, heights)


def test_terrain_fixture_range(heights):
    h = heights[:512, :512]
    assert (h.min(), h.max()) == (-17, 80)          # SURVEY App. B "raw noise heights -17..80"
    top = np.maximum(16, np.minimum(512, h))
    assert int((top - 1).sum()) == 8583552          # solid voxels at 512^3


def test_lsvo_512_layout(nodes9):
    n = nodes9
    assert len(n) == 10528393 and len(n) * 8 == 84227144
    assert int((n["child_mask"] != 0).sum()) == 1316049
    assert int(n["child_offset"].max()) == 7883537
    first = [(int(a["child_mask"]), int(a["leaf_mask"]), int(a["child_offset"])) for a in n[:5]]
    assert first == [(204, 0, 1), (0, 0, 0), (0, 0, 0), (51, 0, 6), (51, 0, 5283557)]
    assert np.all(n["color"] == 1)
    # level histogram of non-empty internal nodes
    level = np.zeros(len(n), np.int8)
    counts = []
    frontier = np.array([0], np.int64)
    for lv in range(9):
        counts.append(len(frontier))
        nd = n[frontier]
        nxt = []
        for k in range(8):
            sel = ((nd["child_mask"] >> k) & 1).astype(bool) & ~((nd["leaf_mask"] >> k) & 1).astype(bool)
            nxt.append(frontier[sel] + nd["child_offset"][sel].astype(np.int64) + k)
        frontier = np.concatenate(nxt)
    assert counts == [1, 4, 16, 94, 537, 3220, 21166, 151272, 1139739]


def test_lsvo_other_depths(heights):
    assert len(O.compile_terrain(8, heights)) == 2646233        # 20.19 MiB


def _frame(nodes9, textures, pitch):
    top, side = textures
    W, H = 960, 540
    light = np.array([-200, -1000, -300], np.float32) * np.float32(1 / 512) + np.float32(1)
    cam = O.make_camera((256, 200, 256), O.make_rotation(0.0, pitch), 1.0, 0.0, 1.0)  # Camera defaults
    p = O.make_params(W, H, light, use_gi=0, use_samples=1, shadow_samples=1)
    _, _, prim, st = O.render_frame(nodes9, 9, top, side, cam, p, want_prim=True, threads=8)
    return prim, st


def test_primary_rays_pitch_m05(nodes9, textures):
    prim, _ = _frame(nodes9, textures, -0.5)
    c = prim["complexity"]
    hit = prim["hit"] != 0
    assert int(hit.sum()) == 514400
    assert round(float(c.mean()), 2) == 38.39
    assert [int(np.percentile(c, q)) for q in (50, 90, 99)] == [35, 59, 87]
    assert int(c.max()) == 147
    n = prim["normal"][hit]
    nx = n[:, 0] != 0
    ny = ~nx & (n[:, 1] != 0)
    nz = ~nx & ~ny & (n[:, 2] != 0)
    assert (int(nx.sum()), int(ny.sum()), int(nz.sum())) == (100924, 225631, 187845)
    assert int(((n != 0).sum(1) > 1).sum()) == 10           # multi-axis normals
    # sample hit at lens (0, 0.2) = pixel (480, 378)
    h = prim[378 * 960 + 480]
    assert np.allclose(h["position"], [1.5, 1.46875, 1.59325], atol=2e-6)
    assert h["normal"].tolist() == [-0.0, -2.0, -0.0] and np.signbit(h["normal"]).all()
    assert abs(float(h["distance"]) - 0.121648) < 1e-6 and int(h["complexity"]) == 31


def test_primary_rays_other_poses(nodes9, textures):
    prim, _ = _frame(nodes9, textures, 0.0)
    c = prim["complexity"]
    assert int((prim["hit"] != 0).sum()) == 263162
    assert round(float(c.mean()), 2) == 32.33 and int(c.max()) == 147
    n = prim["normal"][prim["hit"] != 0]
    assert int(((n != 0).sum(1) > 1).sum()) == 1389
    prim, _ = _frame(nodes9, textures, -1.2)
    c = prim["complexity"]
    assert int((prim["hit"] != 0).sum()) == 518400
    assert round(float(c.mean()), 2) == 24.37 and int(c.max()) == 106


def test_misses_are_zeroed(nodes9):
    org = np.array([[1.5, 1.1, 1.5]], np.float32)
    d = np.array([[0.0, -1.0, 0.0]], np.float32)     # straight up into the sky
    h = O.cast_rays(nodes9, 9, org, d)[0]
    assert h["hit"] == 0 and h["complexity"] > 0
    assert not h["position"].any() and not h["normal"].any() and h["distance"] == 0


def test_rng_quantisation():
    L = O.lib()
    vals = {L.orc_get_rand_counter(k, -0.5, 0.5) for k in range(1000)}
    assert len(vals) == 100                           # utils.cpp:77-81: 100 levels
    assert min(vals) == -0.5 and max(vals) < 0.5
    # xorshf96 first outputs (LP64 unsigned long)
    L.orc_xorshf96_reset()
    a = [L.orc_xorshf96() for _ in range(3)]
    x, y, z = 123456789, 362436069, 521288629
    exp = []
    M = (1 << 64) - 1
    for _ in range(3):
        x ^= (x << 16) & M; x ^= x >> 5; x ^= (x << 1) & M
        t = x; x = y; y = z; z = t ^ x ^ y
        exp.append(z)
    assert a == exp


def test_frac_matches_modf():
    L = O.lib()
    for v in (0.0, 0.25, 513.75, 1023.999, -2.5, -0.0, 7.0):
        assert L.orc_frac(v) == np.float32(np.modf(np.float32(v))[0])


def test_scene_cameras_are_in_free_space(heights, textures):
    """The benchmark cameras (scenes.reference_camera_position) must not sit inside
    solid voxels: every primary hit has a non-zero normal."""
    import cpuvoxelraycaster_amd as vrc
    top, side = textures
    for depth in (7, 8):
        nodes = O.compile_terrain(depth, heights)
        cam = O.make_camera(vrc.reference_camera_position(depth), O.make_rotation(0.0, -0.5))
        p = O.make_params(96, 54, vrc.reference_light(depth), use_samples=1, shadow_samples=1)
        _, _, prim, _ = O.render_frame(nodes, depth, top, side, cam, p, want_prim=True, threads=4)
        hit = prim["hit"] != 0
        assert hit.sum() > 1000 and (np.abs(prim["normal"][hit]).sum(1) > 0).all()


def test_nan_ray_is_a_miss(nodes9):
    h = O.cast_rays(nodes9, 9, np.array([[1.5, 1.4, 1.5]], np.float32), np.array([[np.nan, 0.5, 0.5]], np.float32))[0]
    assert h["hit"] == 0 and h["complexity"] == 0


def test_noise_restatement_equals_real_fastnoise(heights):
    """The one place where the oracle is pinned by running the reference itself: the
    restated SimplexFractal terrain heights equal, for all 1024 x 1024 columns, the
    fixture generated by the reference's own lib/fastnoise/FastNoise.cpp."""
    assert np.array_equal(O.terrain_heights(1024), heights)


def test_noise_restatement_against_live_reference_build(heights):
    """The reference's FastNoise for a 300 x 300 scene against the restatement: run live where oracle/_ref was built (the
    reference mounted), else as recorded from that same library (tests/golden/terrain_height_1024.npz, whose top-left
    S x S block is the S^3 scene's height field, tests/tools/make_golden.py)."""
    import ctypes as C
    import os
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_fastnoise.so")
    if os.path.exists(ref):
        lib = C.CDLL(ref)
        h = np.zeros((300, 300), np.int32)
        lib.ref_terrain_heights(C.c_int32(300), h.ctypes.data_as(C.c_void_p))
        assert np.array_equal(h, heights[:300, :300])
    else:
        h = heights[:300, :300]
    assert np.array_equal(h, O.terrain_heights(300))


def test_reference_probe_sequence_random_and_gi_rays(nodes9):
    """SURVEY App. B's instrumented run of the unmodified reference, replayed draw for
    draw with the restated xorshf96 stream (utils.cpp:11-25, LP64): after 960x540
    getRay calls (2 draws each) it cast 200 000 random rays with origins in [0,3)^3
    (5 025 hits), 100 000 axis rays (2 draws each), and then, on every second pixel of
    the pitch -0.5 frame, one GI ray (coef 0.5) per primary hit: 128 568 primary hits,
    116 671 GI hits = 77 971 LOD cut-offs (per-scale histogram below) + 38 700 leaf hits.
    Pins the RNG restatement, getRand's quantisation, the GI ray construction
    (raycaster.hpp:171-194), the LOD cut (lsvo.hpp:82-85) and walks from outside the cube."""
    f = np.float32
    O.lib().orc_xorshf96_reset()
    O.xorshf96_draws(518400 * 2)
    z = O.xorshf96_draws(200000 * 6).reshape(200000, 6)
    org = O.get_rand(z[:, 0:3], 0, 3)
    dd = (O.get_rand(z[:, 3:6], -1, 1) + f(0.003)).astype(f)
    inv = (f(1) / np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])).astype(f)
    h = O.cast_rays(nodes9, 9, org, (dd * inv[:, None]).astype(f), threads=8)
    assert int((h["hit"] != 0).sum()) == 5025
    O.xorshf96_draws(100000 * 2)
    W, H = 960, 540
    X, Y = np.meshgrid(np.arange(0, W, 2), np.arange(0, H, 2), indexing="ij")      # x outer, y inner
    X, Y = X.reshape(-1).astype(f), Y.reshape(-1).astype(f)
    v = np.stack([X / f(H) - f(W) / f(H) * f(0.5), Y / f(H) - f(0.5), np.ones_like(X)], 1).astype(f)

    def normalize(a):
        i = (f(1) / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])).astype(f)
        return (a * i[:, None]).astype(f)

    r = normalize(normalize(v))            # focal_length 1, aperture 0 (camera_controller.hpp:39-42)
    m = O.make_rotation(0.0, -0.5)
    d = np.stack([(m[0] * r[:, 0] + m[1] * r[:, 1]) + m[2] * r[:, 2], (m[3] * r[:, 0] + m[4] * r[:, 1]) + m[5] * r[:, 2],
                  (m[6] * r[:, 0] + m[7] * r[:, 1]) + m[8] * r[:, 2]], 1).astype(f)
    o = np.tile(np.array([256, 200, 256], f) * f(1 / 512) + f(1), (len(d), 1)).astype(f)
    prim = O.cast_rays(nodes9, 9, o, d, threads=8)
    hit = prim["hit"] != 0
    assert int(hit.sum()) == 128568
    # draws: 2 per getRay, then c1, c2 for pixels whose primary ray hit
    per_pixel = np.where(hit, 4, 2)
    z = O.xorshf96_draws(int(per_pixel.sum()))
    first = np.concatenate([[0], np.cumsum(per_pixel)[:-1]])
    c1 = O.get_rand(z[first[hit] + 2], -1000, 1000)
    c2 = O.get_rand(z[first[hit] + 3], -1000, 1000)
    hp = prim[hit]
    n = hp["normal"]
    nn = f((f(1.0) / f(512.0)) * f(0.0078125) * f(2.0))
    noise = np.zeros_like(n)
    mx = n[:, 0] != 0
    my = ~mx & (n[:, 1] != 0)
    mz = ~mx & ~my
    noise[mx, 1], noise[mx, 2] = c1[mx], c2[mx]
    noise[my, 0], noise[my, 2] = c1[my], c2[my]
    noise[mz, 0], noise[mz, 1] = c1[mz], c2[mz]
    g = O.cast_rays(nodes9, 9, (hp["position"] + n * nn).astype(f), normalize(((n + noise).astype(f) * nn).astype(f)),
                    coef=0.5, bias=0.0, threads=8)
    kind, sc = g["hit"] & 0xff, (g["hit"] >> 16) & 0xff
    assert (int((kind != 0).sum()), int((kind == 2).sum()), int((kind == 1).sum())) == (116671, 77971, 38700)
    hist = [int(((kind == 2) & (sc == s)).sum()) for s in range(14, 22)]
    assert hist == [12775, 13589, 14068, 16431, 14450, 3836, 2805, 17]


def _host_replay_reader(tmp_path):
    """The product's reader: vrc_host::readReplay (host/hip_raycaster.hpp), as a tiny executable."""
    import subprocess
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n#include <cstdio>\n#include <cstring>\nint main(int c, char** v){ auto l = vrc_host::readReplay(v[1]);'
           'std::printf("%%zu", l.size()); for (auto& e : l) { float f[6] = {e.time, e.pose.position.x, e.pose.position.y, e.pose.position.z, e.pose.view_angle.x, e.pose.view_angle.y};'
           'for (float q : f) { unsigned u; std::memcpy(&u, &q, 4); std::printf(" %%u", u); } } return 0; }\n') % hdr
    exe = str(tmp_path / "replay_reader")
    subprocess.run(["g++", "-std=c++14", "-x", "c++", "-", "-o", exe, "-L" + os.path.join(ROOT, "cpuvoxelraycaster_amd"),
                    "-l:libvrc_hip.so", "-Wl,-rpath," + os.path.join(ROOT, "cpuvoxelraycaster_amd")], input=src.encode(), check=True)

    def read(path):
        out = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.split()
        vals = [int(v) for v in out[1:]]
        assert len(vals) == 6 * int(out[0])
        return [vals[i:i + 6] for i in range(0, len(vals), 6)]
    return read


def test_replay_reader_pinned_by_reference_execution(built, tmp_path):
    """N3: tests/golden/replay_cases.json holds what the reference's own ReplayElements::loadFromFile
    (include/replay.hpp, compiled where it lies: oracle/_ref/libref_replay.so, tests/tools/make_golden_replay.py) parses from
    a set of replay texts -- ticks spanning lines, numbers glued to text, truncated and malformed ticks, float32
    overflow, nan / hex words.  The host adapter's reader and the Python replay driver must return the same ticks bit
    for bit; where /root/reference is mounted the live reference reader is checked against the fixture too."""
    import ctypes as C
    import json
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay_bench
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "replay_cases.json")))
    assert len(cases) >= 10
    read_host = _host_replay_reader(tmp_path)
    ref = None
    ref_lib = os.path.join(ROOT, "oracle", "_ref", "libref_replay.so")
    if os.path.isdir("/root/reference") and os.path.exists(ref_lib):
        ref = C.CDLL(ref_lib)
        ref.ref_replay_load.restype = C.c_int32
        ref.ref_replay_load.argtypes = [C.c_char_p, C.c_void_p, C.c_int32]
    for name, case in cases.items():
        path = str(tmp_path / (name + ".replay"))
        with open(path, "w") as f:
            f.write(case["text"])
        want = case["ticks_f32_bits"]
        assert read_host(path) == want, name
        got_py = np.array(replay_bench.load_replay(path), np.float32).reshape(-1, 6).view(np.uint32).tolist()
        assert got_py == want, name
        if ref is not None:
            buf = np.zeros((64, 6), np.float32)
            n = ref.ref_replay_load(path.encode(), buf.ctypes.data, 64)
            assert buf[:n].view(np.uint32).tolist() == want, name
    missing = str(tmp_path / "does_not_exist.replay")
    assert read_host(missing) == [] and replay_bench.load_replay(missing) == []


def test_frame_on_the_references_own_swarm_pool(heights, textures):
    """The oracle's per-area job (the swarm lambda's body, main.cpp:139-152) on the REAL swrm::Swarm of the reference
    (lib/swarm/swarm.hpp, compiled where it lies into oracle/_ref): 16 workers, static 4 x 4 areas -- same accumulators
    and counters as orc_render_frame on the pixels the reference's decomposition covers, frame after frame (the pool's
    silent job drop, swarm.hpp:221-223, is retried by the shim).  Where oracle/_ref is not built (the reference not mounted)
    the pool's recorded output stands in for the live run (tests/golden/swarm_frames_d7_162x91.npz,
    tests/tools/make_golden_swarm.py); where it is, the live run must also equal that record."""
    import cpuvoxelraycaster_amd as vrc
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import make_golden_swarm as G
    depth, W, H = G.DEPTH, G.W, G.H                # W, H not multiples of 4: the reference never renders the remainder
    assert (depth, W, H, G.FRAMES) == (7, 162, 91, 6)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "swarm_frames_d7_162x91.npz"))
    if O.RefSwarm.available():
        acc, rays, steps = G.swarm_frames(O, heights, textures)
        assert np.array_equal(acc, gold["accum"]) and (rays, steps) == (int(gold["rays"]), int(gold["sum_complexity"]))
    else:
        acc, rays, steps = gold["accum"].astype(np.uint32), int(gold["rays"]), int(gold["sum_complexity"])
    nodes = O.compile_terrain(depth, heights)
    top, side = textures
    cam = O.make_camera(vrc.reference_camera_position(depth), O.make_rotation(0.0, -0.5))
    light = vrc.reference_light(depth)
    oacc = None
    orays = osteps = 0
    for s in range(6):
        p = O.make_params(W, H, light, use_gi=1, use_samples=1, shadow_samples=1, frame_index=s)
        _, oacc, _, ost = O.render_frame(nodes, depth, top, side, cam, p, accum=oacc, threads=4)
        orays, osteps = orays + ost.rays, osteps + ost.sum_complexity
    cw, ch = 4 * (W // 4), 4 * (H // 4)
    assert np.array_equal(acc[:ch, :cw], oacc[:ch, :cw])
    assert not acc[ch:].any() and not acc[:, cw:].any()
    assert (acc[:ch, :cw, 3] == 6).all()
    assert 0 < rays <= orays and 0 < steps <= osteps


def test_grid_start_cell_conversion_rule():
    """grid_3d.hpp:58-60 `(int)position.x` is undefined in C for NaN and outside [-2^31, 2^31); the reference as shipped
    (x86-64) yields INT_MIN for all of them, so such a ray starts nowhere: a miss with a zero record.  orc_grid_cell states
    that rule instead of leaving it to a compiler; the kernel follows the same one (tests/test_gpu_grid.py)."""
    import ctypes as C
    L = O.lib()
    L.orc_grid_cell.restype = C.c_int32
    L.orc_grid_cell.argtypes = [C.c_float]
    INT_MIN = -2 ** 31
    f = np.float32
    for v, cell in ((np.nan, INT_MIN), (-np.nan, INT_MIN), (np.inf, INT_MIN), (-np.inf, INT_MIN), (2.0 ** 31, INT_MIN),
                    (-2.0 ** 31, INT_MIN), (3e9, INT_MIN), (-3e9, INT_MIN), (np.finfo(f).max, INT_MIN),
                    (2.0 ** 31 - 128, 2 ** 31 - 128), (-2.0 ** 31 + 128, -2 ** 31 + 128),
                    (-0.5, 0), (-0.0, 0), (-0.999, 0), (-1.0, -1), (-1.5, -1), (0.0, 0), (0.999, 0), (7.5, 7), (8.0, 8)):
        assert L.orc_grid_cell(f(v)) == cell, v
    # through the cast: a solid 8^3 grid, direction +x
    cells = np.ones((8, 8, 8), np.uint8)
    d = np.asarray([1.0, 0.0, 0.0], f)
    for v in (np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 3e9, 2.0 ** 31 - 128):
        for a in range(3):
            org = np.asarray([3.5, 3.5, 3.5], f)
            org[a] = v
            assert not O.grid_cast_rays(cells, org[None], d[None]).view(np.uint8).any(), (v, a)
        assert not O.grid_cast_rays(cells, np.full((1, 3), v, f), d[None]).view(np.uint8).any(), v
    # -0.5 truncates to cell 0 and so walks: the first new cell, x = 1, is the hit
    h = O.grid_cast_rays(cells, np.asarray([[-0.5, 3.5, 3.5]], f), d[None])[0]
    assert (h["hit"], h["node"], h["complexity"], h["distance"]) == (1, (1 * 8 + 3) * 8 + 3, 1, 1.5)
    assert h["position"].tolist() == [1.0, 3.5, 3.5] and h["normal"].tolist() == [-1.0, 0.0, 0.0]
