"""The frame launch planner (csrc/vrc_plan.h) called on the host: which build of the frame-kernel table a launch gets, how the
frame is cut into work units and how large the grid is.  tests/cpp/frame_plan_main.cpp includes the planner, links the built
library for the real kernel table and makes no HIP call, so none of this needs a device.  Expected values come from the
project's record -- the kernels tests/test_gpu_occupancy.py asserts on the GPU; if the two ever disagree the planner has become
device-dependent -- and from tests/golden/frame_plans.txt, the plans of the last render_impl that planned inline (its planning
text in a throw-away harness over tools/frame_plan_cases.py's sweep, 2 330 560 cases; this file is the fixed-seed sample
`frame_plan_cases.py sample` of them)."""
import os
import re
import subprocess
import sys

import pytest

from cpuvoxelraycaster_amd import build

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

FIELDS = ("rc", "kernel", "grid", "lds", "n_items", "sample_chunk", "sample_chunk_tail", "tail_tiles", "checker_wide",
          "spp", "row_block", "shard_index", "shard_count")


@pytest.fixture(scope="module")
def planner(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan_main")
    subprocess.check_call([HIPCC, "-std=c++17", "-Wall", "-Werror", "-x", "hip", "--cuda-host-only",
                           os.path.join(ROOT, "tests", "cpp", "frame_plan_main.cpp"),
                           "-L" + build.PKG, "-lvrc_hip", "-Wl,-rpath," + build.PKG, "-o", exe])

    def run(cases):
        r = subprocess.run([exe], input="".join(c + "\n" for c in cases), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return lines
    return run


def case(pinhole=1, gi_bounces=1, use_samples=1, spp=4, checker=-1, fused=0, capture=0, size=(1920, 1080), depth=9, shard=(0, 0, 1),
         blocks_per_cu=0, sample_chunk=0, tail_units=4, lane_samples=0, quad_walks=1, reuse=0, from_root=0, cu_count=256):
    """one input line of frame_plan_main (tools/frame_plan_cases.py names the columns); the defaults are a new renderer's"""
    return " ".join(str(int(v)) for v in (pinhole, gi_bounces, use_samples, spp, checker, fused, capture, *size, depth, *shard,
                                          blocks_per_cu, sample_chunk, tail_units, lane_samples, quad_walks, reuse, from_root, cu_count))


def test_library_choice_at_baseline_size(planner):
    """the ten rows of tests/test_gpu_occupancy.py::test_library_choice_at_baseline_size (1920x1080, depth 9, the MI355X's 256 CUs),
    and the 6-wave plain build that test compares each of them with"""
    rows = [  # pinhole, whole-spp units, spp, bounces, expected kernel (use_gi does not reach the planner)
        (1, False, 4, 1, "k_render_sync_pinhole_s4"),
        (1, True, 4, 1, "k_render_sync_pinhole_q"),
        (1, True, 4, 1, "k_render_sync_pinhole_q"),
        (1, False, 1, 1, "k_render_sync_pinhole"),
        (0, False, 4, 1, "k_render_sync_s4"),
        (0, True, 4, 1, "k_render_sync_w7"),
        (0, False, 4, 1, "k_render_sync_s4"),
        (1, True, 4, 2, "k_render_sync_pinhole2_q"),
        (1, False, 4, 2, "k_render_sync_pinhole2"),
        (0, True, 4, 2, "k_render_sync2"),
    ]
    mine = [case(pinhole=pin, spp=n, gi_bounces=b, sample_chunk=n if whole else 0) for pin, whole, n, b, _ in rows]
    plain = [case(pinhole=pin, spp=n, gi_bounces=b, sample_chunk=n if whole else 0, blocks_per_cu=6, lane_samples=1, quad_walks=0)
             for pin, whole, n, b, _ in rows]
    got, base = planner(mine), planner(plain)
    for (pin, _, _, b, kernel), g, p in zip(rows, got, base):
        assert g.split()[:2] == ["0", kernel], (kernel, g)
        assert p.split()[:2] == ["0", ("k_render_sync_pinhole" if pin else "k_render_sync") + ("2" if b == 2 else "")], p


def test_forced_builds(planner):
    """tests/test_gpu_occupancy.py::test_forced_builds_equal_the_oracle: 161x93, depth 7, 3 spp, vrc_renderer_set_tuning(blocks_per_cu)
    3 / 6 / 7 / 8, fused or not: the 6-wave build of the kind, and the lens kernel's 7-wave build from 7 on (vrc_internal.h)"""
    for pin, base in ((1, "k_render_sync_pinhole"), (0, "k_render_sync")):
        names = set()
        for blocks in (3, 6, 7, 8):
            for fused in (0, 1):
                out, = planner([case(pinhole=pin, spp=3, size=(161, 93), depth=7, blocks_per_cu=blocks, fused=fused)])
                want = base + ("_resolved" if fused else "") + ("_w7" if not pin and blocks >= 7 else "")
                assert out.split()[:2] == ["0", want], (blocks, fused, out)
                names.add(want)
        assert names == {base, base + "_resolved"} | (set() if pin else {base + "_w7", base + "_resolved_w7"})


def test_plans_equal_the_inline_planner_they_were_taken_from(planner):
    """every line of tests/golden/frame_plans.txt; and the fixture itself keeps what it was sampled for: every row of the
    frame-kernel table, both planner errors, a shard that owns no row block, and launches that qualify for the quadrant walks
    except for their units' samples (planned again for the plain build)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import frame_plan_cases as fpc
    with open(os.path.join(ROOT, "tests", "golden", "frame_plans.txt")) as f:
        pairs = [line.rstrip("\n").split(" => ") for line in f if line.strip()]
    cases, plans = [c for c, _ in pairs], [p for _, p in pairs]
    table = set(re.findall(r"\bX\((k_render_sync\w*),", open(os.path.join(build.CSRC, "vrc_kernels.hip")).read()))
    assert len(table) >= 26 and {p.split()[1] for p in plans if p.startswith("0 k_")} == table
    assert any(p == "-1 error: vrc_render_frame: frame too large" for p in plans)
    assert any(p.startswith("-1 error: vrc_render_frame: ") and "work units (tiles x sample chunks) do not fit 32 bits" in p for p in plans)
    assert any(p.startswith("0 - ") for p in plans)
    fallbacks = [c for c, p in pairs if fpc.quad_fallback(c, p)]
    assert fallbacks and any(c.split()[3] == "12" and c.split()[14] == "0" for c in fallbacks)     # 12 spp, automatic chunk
    assert all(len(p.split()) == len(FIELDS) for p in plans if p.startswith("0 "))
    got = planner(cases)
    wrong = [(c, p, g) for c, p, g in zip(cases, plans, got) if p != g]
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ, the first: {wrong[0]}"
