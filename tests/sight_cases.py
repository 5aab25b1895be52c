"""The case generators of the sight tests: tests/test_gpu_sight.py runs them on the device, tests/test_sight_host.py holds
them to their conditions on the CPU (a stride case must give the stride room and must end both ways often enough)."""
import functools

import numpy as np

import distance_model
import sight_model as model

STRIDE_LOS = (1, 2, 3, 5, 7, 26, 27)          # non-squares: the rounding of both square roots
STRIDE_SIZE, STRIDE_DENSITY, STRIDE_RANDOM, STRIDE_AIMED = 64, 0.002, 4096, 640
# (name, to_empty, outside): the field to the solid, the same with the volume's faces as features, and the field to the empty
STRIDE_FIELDS = (("solid", False, False), ("solid_outside", False, True), ("empty", True, False))
TIE_DIRECTIONS = ((1, 1, 1), (1, 1, 0), (2, 2, 1), (3, 1, 0), (4, 2, 2))


def random_solid(S, density, seed):
    return (np.random.default_rng(seed).random((S, S, S)) < density).astype(np.uint8)


def starts_to_all(S, starts):
    """(len(starts) * S^3, 6): every segment from each start to every voxel"""
    ends = np.indices((S, S, S)).reshape(3, -1).T
    return np.concatenate([np.concatenate([np.tile(np.asarray(s), (len(ends), 1)), ends], 1) for s in starts]).astype(np.int32)


def mirrors(direction):
    """the direction under every permutation of its axes and every choice of signs, each once"""
    from itertools import permutations, product
    out = set()
    for perm in permutations(direction):
        for signs in product((1, -1), repeat=3):
            out.add(tuple(p * s for p, s in zip(perm, signs)))
    return sorted(out)


def tie_segments(S=16):
    """(n, 6): from the centre voxel along every mirror of TIE_DIRECTIONS, as many whole multiples as fit, both ways round"""
    c = S // 2
    segs = []
    for direction in TIE_DIRECTIONS:
        for d in mirrors(direction):
            k = min((c - 1) // abs(v) for v in d if v)
            a, b = (c, c, c), tuple(c + k * v for v in d)
            segs += [a + b, b + a]
    return np.array(segs, np.int32)


def diagonal_pair_cases(S=16):
    """Two solids that touch diagonally, the segment through what they share.  (solid, a, b, thin, touch) with the expected
    (status, at, before) of both modes on the field to the solid, lo = 1."""
    c = S // 2
    cases = []
    # an edge: solids at (c+1, c, c) and (c, c+1, c); the segment (c, c, c) -> (c+1, c+1, c) passes through their shared edge
    solid = np.zeros((S, S, S), np.uint8)
    solid[c + 1, c, c] = solid[c, c + 1, c] = 1
    a, b = (c, c, c), (c + 1, c + 1, c)
    cases.append((solid, a, b, (model.CLEAR, b, a), (model.BLOCKED, (c + 1, c, c), a)))
    # a corner: solids at (c+1, c+1, c) and (c, c, c+1) share the corner the segment (c, c, c) -> (c+1, c+1, c+1) passes
    # through; the supercover meets (c+1, c, c), (c, c+1, c) first (masks 1, 2), then (c+1, c+1, c) (mask 3)
    solid = np.zeros((S, S, S), np.uint8)
    solid[c + 1, c + 1, c] = solid[c, c, c + 1] = 1
    a, b = (c, c, c), (c + 1, c + 1, c + 1)
    cases.append((solid, a, b, (model.CLEAR, b, a), (model.BLOCKED, (c + 1, c + 1, c), (c, c + 1, c))))
    return cases


def stride_solid(seed, S=STRIDE_SIZE, density=STRIDE_DENSITY):
    """single-voxel obstacles, density * S^3 of them, all in the slab x < S/8: the rest is the open space in which a walk has
    room to stride, so that a case exercises both the jumps and the plain steps between close obstacles"""
    rng = np.random.default_rng(seed)
    n = int(round(density * S ** 3))
    solid = np.zeros((S, S, S), np.uint8)
    slab = np.indices((S // 8, S, S)).reshape(3, -1).T
    pick = slab[rng.choice(len(slab), n, replace=False)]
    solid[pick[:, 0], pick[:, 1], pick[:, 2]] = 1
    return solid


def stride_segments(solid, seed, n_random=STRIDE_RANDOM, n_aimed=STRIDE_AIMED, margin=6):
    """(n_random + 8 n_aimed, 6).  Random segments between voxels at least `margin` from every face (a ball of lo <= 27 fits
    there on a field with outside != 0).  Then, for n_aimed obstacles o, four aimed ones: with a small step d that points
    into the open space, a = m - i d and b = m + j d, i and j as large as the volume allows (i <= 2), run through the centre
    of m exactly -- m = o twice, with two steps (hits), and m = the neighbour of o on either side along a random axis
    (grazes by one voxel).  Then the same 4 n_aimed segments from b to a: a long approach through the open space that ends at
    the obstacle, which is where a jump that is too long would pass it."""
    S = solid.shape[0]
    rng = np.random.default_rng(seed)
    segs = [rng.integers(margin, S - margin, (n_random, 6))]
    obstacles = np.argwhere(solid)
    for o in obstacles[rng.integers(0, len(obstacles), n_aimed)]:
        axis = int(rng.integers(0, 3))
        for side in (-1, 0, 0, 1):
            m = o.copy()
            m[axis] = min(max(m[axis] + side, 0), S - 1)
            d = np.array([rng.integers(1, 4), rng.integers(-3, 4), rng.integers(-3, 4)])
            i = min([2] + [int(m[c] // d[c]) if d[c] > 0 else int((S - 1 - m[c]) // -d[c]) for c in range(3) if d[c]])
            j = min(int((S - 1 - m[c]) // d[c]) if d[c] > 0 else int(m[c] // -d[c]) for c in range(3) if d[c])
            segs.append(np.concatenate([m - i * d, m + j * d])[None, :])
    away = np.concatenate(segs[1:])
    return np.concatenate([segs[0], away, away[:, [3, 4, 5, 0, 1, 2]]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def stride_case(name, seed=11):
    """(volume, to_empty, outside, D, segments) of one of STRIDE_FIELDS: the occupancy to upload, how its field is made, the
    field by the numpy model, and the segments.  With to_empty the volume is the complement -- the obstacles are its only
    empty voxels -- so that the obstacles are the features either way."""
    to_empty, outside = next((t, o) for n, t, o in STRIDE_FIELDS if n == name)
    solid = stride_solid(seed)
    volume = (1 - solid).astype(np.uint8) if to_empty else solid
    return volume, to_empty, outside, distance_model.field(volume, to_empty, outside), stride_segments(solid, seed + 1)


@functools.lru_cache(maxsize=None)
def stride_visited(touch, seed=11):
    """the visited voxels of the stride segments (the same for every field of STRIDE_FIELDS), walked once per mode"""
    return model.visited_arrays(stride_segments(stride_solid(seed), seed + 1), touch)


def room_to_stride(D, visited, lo):
    """per segment: whether the plain walk passes a clear voxel with isqrt(D) - ceil(sqrt(lo)) >= 2 (hi = NONE)"""
    need = max((model.root_above(lo) + 2) ** 2, lo)
    return np.array([bool((D[w[:, 0], w[:, 1], w[:, 2]] >= need).any()) for w in visited])


def wall_case(S=32):
    """a wall across the volume at x = S/2 with a door far from the straight line: (solid, a, b) for shortestPath / smoothPath"""
    solid = np.zeros((S, S, S), np.uint8)
    solid[S // 2, :, :] = 1
    solid[S // 2, 2:5, 2:5] = 0
    return solid, (4, S - 6, S - 6), (S - 5, S - 6, S - 6)
