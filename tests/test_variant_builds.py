"""The documented experiment builds still compile (round-5 advice: quad_waves() named a macro that only the product build
defined, so every -DVRC_PROBE / -DVRC_WALK_CPP / -DVRC_NO_START_BELOW build was broken without anyone noticing).  A front-end
pass (hipcc -fsyntax-only: host AND gfx950 device side, inline-asm constraints included) of the sources that carry
switches (the kernels; the renderer, through the planner in vrc_plan.h) and the rest of the C ABI, once per flag of cpuvoxelraycaster_amd/build.py's VARIANT_FLAGS; about a second each, no GPU."""
import os
import re
import subprocess

import pytest

from cpuvoxelraycaster_amd import build

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FRONT = [f for f in build.FLAGS if f not in ("-shared", "-fPIC", "-O3")] + ["-fsyntax-only", "-Werror=implicit-function-declaration"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("flag", [""] + build.VARIANT_FLAGS)
def test_variant_flag_compiles(flag):
    for src in ("vrc_kernels.hip", "vrc_renderer.cpp", "vrc_api.cpp", "vrc_ipc.cpp"):
        cmd = [HIPCC] + FRONT + ([flag] if flag else []) + ["-x", "hip", os.path.join(build.CSRC, src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-3000:]}"


def test_variant_builds_have_no_quadrant_kernels_and_say_so():
    """the variants that leave the quadrant-walk kernels out must report it (vrc::quad_available), so that the planner neither
    chooses a quadrant-walk build nor sizes the grid for a build it could not launch"""
    src = open(os.path.join(build.CSRC, "vrc_kernels.hip")).read()
    plan = open(os.path.join(build.CSRC, "vrc_plan.h")).read()
    assert "bool quad_available()" in src and "vrc::quad_available() &&" in plan
    # the occupancy macro is defined whatever the variant
    head = src[:src.index("#define VRC_HAVE_QUAD 1")]
    assert "#define VRC_SYNC_Q_WAVES 6" in head and head.rstrip().endswith("defined(VRC_NO_START_BELOW))")


def test_variant_builds_have_no_quadrant_rows_in_the_frame_kernel_table():
    """the variants that leave the quadrant-walk kernels out have no quadrant rows in the frame-kernel table (vrc::frame_kernel),
    and the planner (vrc_plan.h) chooses only from rows that exist, so that render_impl (vrc_renderer.cpp) neither picks a quadrant
    build nor sizes the grid for a build launch_render could not launch"""
    src = open(os.path.join(build.CSRC, "vrc_kernels.hip")).read()
    plan = open(os.path.join(build.CSRC, "vrc_plan.h")).read()
    renderer = open(os.path.join(build.CSRC, "vrc_renderer.cpp")).read()
    guard = "#if !(defined(VRC_WALK_CPP) || defined(VRC_PROBE) || defined(VRC_NO_START_BELOW))"
    i = src.index(guard)
    j = src.index("#else", i)
    k = src.index("#endif", j)
    # every quadrant row of the one list sits behind the guard, and the other branch has none
    quad_rows = re.findall(r"X\((k_render_sync\w+),[^)]*LaneMap::quad", src)
    assert len(quad_rows) == 4 and quad_rows == re.findall(r"X\((k_render_sync\w+),[^)]*LaneMap::quad", src[i:j])
    assert src[j:k].split() == ["#else", "#define", "VRC_QUAD_FRAME_KERNELS(X)"]
    # the kernels and the table come from that list; the planner asks the table for a quadrant build and launches what it chose
    assert "VRC_FRAME_KERNELS(VRC_FRAME_KERNEL)" in src and "VRC_FRAME_KERNELS(VRC_FRAME_ROW)" in src
    assert "if (k.v.map == LaneMap::quad) return true;" in src and "vrc::quad_available() &&" in plan
    assert "kernel = vrc::frame_kernel(v);" in plan and "vrc::launch_render(*plan.kernel," in renderer
    # the occupancy macro is defined whatever the variant
    assert "#define VRC_SYNC_Q_WAVES 6" in src[:i]
    if os.path.exists(HIPCC):   # and the preprocessor agrees, per variant
        for flag in ("", "-DVRC_WALK_CPP", "-DVRC_PROBE", "-DVRC_NO_START_BELOW"):
            cmd = [HIPCC] + [f for f in FRONT if f != "-fsyntax-only"] + ([flag] if flag else []) + \
                  ["--cuda-host-only", "-E", "-x", "hip", os.path.join(build.CSRC, "vrc_kernels.hip")]
            out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
            assert all((name in out) == (flag == "") for name in quad_rows), flag


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_frame_kernels_keep_their_register_budgets_and_the_committed_record_is_current():
    """round-5 advice: the quadrant-walk kernels sit at the 80-VGPR budget of 6 waves per SIMD; scratch traffic inside the unit
    loop of the timed kernel would cost time without failing any parity test.  The compiler's metadata of THIS tree (device
    side of csrc/vrc_kernels.hip, product flags) against the accepted spills of tools/code_objects.py, and against the newest
    committed profiles/rNN/code_objects.txt (what DESIGN.md and the bench notes quote)."""
    import glob
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import code_objects as co
    rows = co.kernel_rows(extra_flags=[])
    by_name = {r[0]: r for r in rows}
    for name, (spills, scratch) in co.ACCEPTED_SPILLS.items():
        _, vgprs, vspill, _, _, scr = by_name[name]
        assert vspill <= spills and scr <= scratch, (name, vspill, scr, "accepted", spills, scratch)
        assert vgprs <= (72 if name.endswith("_w7") else 80), (name, vgprs)          # 7 / 6 waves per SIMD of 512 VGPRs
    # no frame kernel outside the table spills more than the lens kernels do
    assert all(r[5] <= 72 for r in rows if r[0].startswith("k_render_sync")), [r for r in rows if r[5] > 72]
    newest = sorted(glob.glob(os.path.join(root, "profiles", "r[0-9][0-9]", "code_objects.txt")))[-1]
    assert open(newest).read() == co.table(rows), f"{newest} is not this tree's compiler output: python tools/code_objects.py > {newest}"
