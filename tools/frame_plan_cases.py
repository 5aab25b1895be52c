#!/usr/bin/env python3
"""Input cases for the frame launch planner (csrc/vrc_plan.h), one line of 21 integers each, for tests/cpp/frame_plan_main.cpp:

  pinhole gi_bounces use_samples spp checker_parity fused capture width height depth row_block shard_index shard_count
  blocks_per_cu sample_chunk tail_units_per_wave lane_samples quad_walks reuse_invariant walk_from_root cu_count

  frame_plan_cases.py exhaustive          every combination of the axes that steer a branch, at 1920x1080, depth 9, unsharded, 256 CUs
  frame_plan_cases.py random N SEED       N draws from the whole product
  frame_plan_cases.py fixture             exhaustive + random 1000000 20261016: what tests/golden/frame_plans.txt was sampled from
  frame_plan_cases.py sample CASES PLANS  the fixture ("case => plan" lines) from such a case file and frame_plan_main's output for it

Combinations that vrc_render_frame* rejects or reroutes before it plans are left out: a fused launch needs use_samples and no
checkerboard (vrc_render_frame_resolved renders a checkerboard frame unfused)."""
import itertools
import random
import sys

SPP = (0, 1, 2, 3, 4, 6, 8, 12, 16, 64, 65536)
SIZES = ((7, 5), (161, 93), (1280, 720), (1920, 1080), (3840, 2160), (32768, 32768))
DEPTHS = (7, 8, 9, 10, 16)
# unsharded; row_block 8 with 2 / 8 / 64 shards at index 0, the last, and 1 (which owns no row block of the 7x5 frame)
SHARDS = ((0, 0, 1),) + tuple((8, i, n) for n in (2, 8, 64) for i in (0, n - 1, 1))
BLOCKS = (0, 3, 6, 7, 8)
CHUNKS = (0, 1, 2, 4, 6, None)     # None = the frame's spp
SEED = 20261016


def planned(use_samples, checker, fused):
    return not fused or (use_samples and checker < 0)


def line(pin, gi, us, spp, cp, fused, cap, size, depth, shard, bpc, chunk, tail, lane, quad, reuse, root, cus):
    return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (
        pin, gi, us, spp, cp, fused, cap, size[0], size[1], depth, shard[0], shard[1], shard[2], bpc,
        spp if chunk is None else chunk, tail, lane, quad, reuse, root, cus)


def exhaustive():
    for pin, gi, us, spp, cp, fused, cap, bpc, chunk, tail, lane, quad, reuse, root in itertools.product(
            (1, 0), (0, 1, 2), (0, 1), SPP, (-1, 0, 1), (0, 1), (0, 1), BLOCKS, CHUNKS, (4, 0), (0, 1, 4), (0, 1), (0, 1), (0, 1)):
        if planned(us, cp, fused):
            yield line(pin, gi, us, spp, cp, fused, cap, (1920, 1080), 9, SHARDS[0], bpc, chunk, tail, lane, quad, reuse, root, 256)


def draws(n, seed):
    rng = random.Random(seed)
    c = rng.choice
    while n:
        us, cp, fused = c((0, 1)), c((-1, 0, 1)), c((0, 1))
        if not planned(us, cp, fused):
            continue
        n -= 1
        yield line(c((1, 0)), c((0, 1, 2)), us, c(SPP), cp, fused, c((0, 1)), c(SIZES), c(DEPTHS), c(SHARDS), c(BLOCKS), c(CHUNKS),
                   c((4, 0)), c((0, 1, 4)), c((0, 1)), c((0, 1)), c((0, 1)), c((256, 64)))


def quad_fallback(case, plan):
    """a launch that qualifies for the quadrant walks but for its units' samples, planned again for the plain build"""
    pin, _, us, spp, cp, _, cap, _, _, depth, _, _, _, _, _, _, lane, quad, reuse, root, _ = map(int, case.split())
    kernel = plan.split()[1]
    return (pin and quad and us and spp and spp % 4 == 0 and not reuse and not cap and not root and cp < 0 and depth >= 8 and
            plan.startswith("0 k_") and not kernel.endswith(("_q", "_s4")))


def sample(cases, plans, per_kind=6, fallbacks=60):
    """a fixed-seed sample: every kernel at every frame size, both errors, the empty shard and the quadrant fall-back"""
    kinds = {}
    for case, plan in zip(cases, plans):
        f = plan.split()
        if quad_fallback(case, plan):
            kind = "fallback"
        elif f[0] != "0":
            kind = "error: frame too large" if "frame too large" in plan else "error: work units"
        else:
            kind = f[1] + " at width " + case.split()[7]
        kinds.setdefault(kind, []).append(case + " => " + plan)
    rng = random.Random(SEED)
    for kind in sorted(kinds):
        rows = kinds[kind]
        yield from rng.sample(rows, min(len(rows), fallbacks if kind == "fallback" else 4 * per_kind if kind[0] == "e" else per_kind))


def main(argv):
    if len(argv) == 4 and argv[1] == "sample":
        with open(argv[2]) as c, open(argv[3]) as q:
            sys.stdout.writelines(l + "\n" for l in sample(c.read().splitlines(), q.read().splitlines()))
        return
    if argv[1:] == ["exhaustive"]:
        gen = exhaustive()
    elif len(argv) == 4 and argv[1] == "random":
        gen = draws(int(argv[2]), int(argv[3]))
    elif argv[1:] == ["fixture"]:
        gen = itertools.chain(exhaustive(), draws(1000000, SEED))
    else:
        sys.exit(__doc__)
    sys.stdout.writelines(l + "\n" for l in gen)


if __name__ == "__main__":
    main(sys.argv)
