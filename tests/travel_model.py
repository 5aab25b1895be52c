"""The travel-distance field of include/vrc.h (vrc_travel_field) in numpy: the yardstick of the GPU tests, itself held
against the definition taken literally in tests/test_volume_travel_host.py.  A breadth-first search by levels over a padded
flat array: a level is a handful of fancy-indexing operations whatever its size, so a 64^3 case takes well under a second
and a 2000-step corridor a second or so."""
import numpy as np

NONE = 0xFFFFFFFF


def medium_set(vol, through_empty):
    """M: the solid voxels, or the empty ones"""
    return (vol == 0) if through_empty else (vol != 0)


def offsets(connectivity):
    """the neighbour steps in ascending (dx, dy, dz) order, dx most significant"""
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = (dx != 0) + (dy != 0) + (dz != 0)
                if k == 1 or (connectivity == 26 and k > 1):
                    out.append((dx, dy, dz))
    assert len(out) == connectivity
    return out


def seeds_in_m(vol, seeds, through_empty):
    return (seeds != 0) & medium_set(vol, through_empty)


def field(vol, seeds, connectivity=6, through_empty=False, step_limit=0):
    """T as (S, S, S) uint32: steps from the nearest seed in M through M, NONE elsewhere and beyond step_limit (0 = none)"""
    S = vol.shape[0]
    P = S + 2
    M = np.zeros((P, P, P), bool)
    M[1:-1, 1:-1, 1:-1] = medium_set(vol, through_empty)
    T = np.full((P, P, P), NONE, np.uint32)
    start = np.zeros((P, P, P), bool)
    start[1:-1, 1:-1, 1:-1] = seeds_in_m(vol, seeds, through_empty)
    Mf, Tf = M.reshape(-1), T.reshape(-1)
    deltas = [(dx * P + dy) * P + dz for dx, dy, dz in offsets(connectivity)]
    frontier = np.flatnonzero(start.reshape(-1))
    Tf[frontier] = 0
    level = 0
    while len(frontier) and (step_limit == 0 or level < step_limit):
        level += 1
        found = []
        for d in deltas:
            q = frontier + d
            q = q[Mf[q] & (Tf[q] == NONE)]
            Tf[q] = level
            found.append(q)
        frontier = np.unique(np.concatenate(found))
    return np.ascontiguousarray(T[1:-1, 1:-1, 1:-1])


def stats(T, n_seeds):
    """(seeds, reached, max_steps, argmax) as vrc_travel_stats reports them"""
    finite = T != NONE
    if not finite.any():
        return n_seeds, 0, 0, (0, 0, 0)
    m = int(T[finite].max())
    first = int(np.flatnonzero(T.reshape(-1) == m)[0])
    S = T.shape[0]
    return n_seeds, int(finite.sum()), m, (first // (S * S), (first // S) % S, first % S)


def select(T, lo, hi):
    return (T >= lo) & (T <= hi)


def trace(T, start, connectivity, capacity=None):
    """(length, (k, 3) route) from `start` as vrc_travel_trace_paths walks it: each next voxel the first neighbour in
    ascending (dx, dy, dz) order whose value is one less; k = min(length, capacity - 1) + 1, 0 for a start without a value"""
    S = T.shape[0]
    p = tuple(int(v) for v in start)
    if not all(0 <= v < S for v in p) or T[p] == NONE:
        return NONE, np.zeros((0, 3), np.uint32)
    t = int(T[p])
    last = t if capacity is None else min(t, capacity - 1)
    if last < 0:
        return t, np.zeros((0, 3), np.uint32)
    route = [p]
    steps = offsets(connectivity)
    for k in range(last):
        for dx, dy, dz in steps:
            q = (p[0] + dx, p[1] + dy, p[2] + dz)
            if all(0 <= v < S for v in q) and int(T[q]) == t - k - 1:
                p = q
                break
        else:
            raise AssertionError(f"no neighbour of {p} holds {t - k - 1}: not a travel field")
        route.append(p)
    return t, np.array(route, np.uint32).reshape(-1, 3)
