"""The cases of tests/test_gpu_volume_sweep_large.py: the two sweep-scheme kernels of the voxel volume, the travel-distance
field (csrc/vrc_travel.hip) and the flood fill (csrc/vrc_flood.hip), at 256^3 -- where k_travel_stats takes a second, third
and fourth grid-stride step, a sweep launches 4096 (travel) or 512 (flood) workgroups, the host loop runs through many
batches of eight sweeps and a route is tens of thousands of steps long.  Beside the scenes: the geometry of those kernels
restated in Python from the code as it stands, each with the line it was read off, so that the host test
(tests/test_volume_sweep_cases_host.py) can hold the scenes to the regime they are meant for.  The expected fields and
regions are travel_model.field's and flood_model.flood's, made once per scene and connectivity and kept sparse (a dense
256^3 field is 64 MiB).  numpy and Python integers only."""
import functools

import numpy as np

import flood_model
import travel_model

NONE = travel_model.NONE
GROUP = 256                          # vrc_travel.hip:69: lanes per workgroup of every kernel of the travel field
TV = 16                              # vrc_travel.hip:66: voxels per travel tile along an axis
FV = 32                              # vrc_flood.hip:26: a flood tile is 16 x 16 x 4 words of 2 x 2 x 8 voxels
STATS_GROUPS_MAX = 4096              # vrc_travel.hip:357
BATCH_MAX = 8                        # vrc_travel.hip:65, vrc_flood.hip:25: sweeps between two reads of the counters
TILE_ITERS = 64                      # vrc_travel.hip:64


# ---- the restated geometry --------------------------------------------------------------------------------------------

def travel_tiles_per_axis(S):
    """vrc_travel.hip:71"""
    return S // TV if S >= TV else 1


def flood_tiles_per_axis(S):
    """vrc_flood.hip:46"""
    return S >> 5 if S >= 32 else 1


def travel_tile_of(xyz, S):
    """vrc_travel.hip:111 (the init pass raises this flag) and :133 (the sweep splits it again): ((x / 16) T + y / 16) T + z / 16"""
    xyz = np.asarray(xyz, np.int64)
    T = travel_tiles_per_axis(S)
    return ((xyz[..., 0] // TV) * T + xyz[..., 1] // TV) * T + xyz[..., 2] // TV


def flood_tile_of(xyz, S):
    """vrc_flood.hip:59-61 and :73 on the word (x / 2, y / 2, z / 8) of a voxel: ((cx / 16) T + cy / 16) T + wz / 4"""
    xyz = np.asarray(xyz, np.int64)
    T = flood_tiles_per_axis(S)
    cx, cy, wz = xyz[..., 0] >> 1, xyz[..., 1] >> 1, xyz[..., 2] >> 3
    return ((cx // 16) * T + cy // 16) * T + wz // 4


def tile_split(tile, T):
    """vrc_travel.hip:133, vrc_flood.hip:73: (tx, ty, tz) = (tile / (T T), (tile / T) % T, tile % T)"""
    tile = np.asarray(tile, np.int64)
    return tile // (T * T), (tile // T) % T, tile % T


def travel_scratch_bytes(depth):
    """vrc_travel.hip:289-293"""
    T = travel_tiles_per_axis(1 << depth)
    return 24 + (3 * T ** 3 + BATCH_MAX) * 4


def flood_scratch_bytes(depth):
    """vrc_flood.hip:186-190"""
    T = flood_tiles_per_axis(1 << depth)
    return (3 * T ** 3 + BATCH_MAX) * 4


def stats_launch(depth):
    """vrc_travel.hip:355-357: (quads, workgroups of k_travel_stats)"""
    quads = 1 << (3 * depth - 2)
    want = (quads + GROUP - 1) // GROUP
    return quads, min(want, STATS_GROUPS_MAX)


def quads_per_lane(depth):
    """the iterations of the loop at vrc_travel.hip:231 that the lanes of the launch take (the same for all: a power of two)"""
    quads, groups = stats_launch(depth)
    return -(-quads // (groups * GROUP))


def stats_lane(xyz, S, groups):
    """(iteration, workgroup, thread) of k_travel_stats that sees voxel xyz: qi = dense index / 4 = blockIdx GROUP + thread
    + iteration gridDim GROUP (vrc_travel.hip:231-237)"""
    x, y, z = (int(v) for v in xyz)
    qi = ((x * S + y) * S + z) // 4
    lanes = groups * GROUP
    return qi // lanes, (qi % lanes) // GROUP, qi % GROUP


def stats_pass(T, groups, drop_later=False, tie="index"):
    """k_travel_stats (vrc_travel.hip:225-252) on a field T under `groups` workgroups: (reached, max, argmax) as the kernel
    combines them -- a lane counts the values of its quads in 32 bits and keeps the largest (value << 32) | ~dense index
    (:237-238), the workgroup takes the largest of its lanes (:241-246) and the sum of their counts (:247), and a 64-bit
    atomic each joins the workgroups (:249-250); decode as decode_argmax of vrc_snapshots.hip does: no value -> (0, 0, (0, 0, 0)).
    For experiments with a wrong kernel: drop_later=True takes only each lane's first quad (a loop that never strides);
    tie="lane" breaks a tie of values by the lower thread, then the lower workgroup, then the earlier iteration -- by who saw
    it, not by where it lies."""
    S = T.shape[0]
    flat = T.reshape(-1)
    lanes = groups * GROUP
    idx = np.flatnonzero(flat != NONE)
    qi = idx // 4
    if drop_later:
        keep = qi < lanes
        idx, qi = idx[keep], qi[keep]
    if not len(idx):
        return 0, 0, (0, 0, 0)
    val = flat[idx].astype(np.uint64)
    lane = qi % lanes
    if tie == "index":
        low = (~idx.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    else:
        assert tie == "lane"
        seen = ((lane % GROUP) * groups + lane // GROUP) * (flat.size // 4 // lanes + 1) + qi // lanes        # below 2^32
        low = (~seen.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    packed = (val << np.uint64(32)) | low
    per_lane_best = np.zeros(lanes, np.uint64)
    np.maximum.at(per_lane_best, lane, packed)
    per_lane_count = np.bincount(lane, minlength=lanes).astype(np.uint32)
    per_group_best = per_lane_best.reshape(groups, GROUP).max(axis=1)
    per_group_count = per_lane_count.reshape(groups, GROUP).sum(axis=1, dtype=np.uint64)
    best, reached = int(per_group_best.max()), int(per_group_count.sum())
    if tie == "lane":                    # the voxel that lane saw: the first (smallest index) with that packed value
        first = int(idx[np.flatnonzero(packed == np.uint64(best))[0]])
    else:
        first = ~best & 0xFFFFFFFF
    return reached, best >> 32, (first // (S * S), (first // S) % S, first % S)


def batches(n_sweeps, max_sweeps=None):
    """the batch sizes of the host loop (vrc_travel.hip:328-350, vrc_flood.hip:225-248) when sweep `n_sweeps` is the first
    to count 0: 2, 4, 8, 8, ... cut at max_sweeps; their sum is the `sweeps` the call reports, and every batch but the first
    is preceded by a reset of the counters (:332)"""
    out, issued, batch = [], 0, 2
    while True:
        b = batch if max_sweeps is None else min(batch, max_sweeps - issued)
        out.append(b)
        issued += b
        if issued >= n_sweeps or issued == max_sweeps:
            return out
        if batch < BATCH_MAX:
            batch *= 2


def crossings(route, S):
    """the changes of travel tile along an ordered (n, 3) route"""
    tiles = travel_tile_of(route, S)
    return int((np.diff(tiles) != 0).sum())


def tile_distance(a, b, connectivity):
    """the fewest changes of travel tile on any chain of neighbours from voxel a to voxel b: a step changes one tile
    coordinate under 6 neighbours (Manhattan), up to three under 26 (Chebyshev)"""
    d = np.abs(np.asarray(a, np.int64) // TV - np.asarray(b, np.int64) // TV)
    return int(d.sum() if connectivity == 6 else d.max())


# ---- corridors: polylines of straight one-voxel runs ----------------------------------------------------------------------

def polyline(corners):
    """(the ordered voxels of the axis-aligned polyline through `corners`, a mask of those at which it turns)"""
    out, turn = [tuple(corners[0])], [False]
    for a, b in zip(corners, corners[1:]):
        a, b = np.array(a), np.array(b)
        step = np.sign(b - a)
        assert (step != 0).sum() == 1
        for k in range(1, int(np.abs(b - a).max()) + 1):
            out.append(tuple((a + k * step).tolist()))
            turn.append(False)
        turn[-1] = True
    turn[-1] = False
    return np.array(out, np.int64), np.array(turn)


def route_of(path, connectivity):
    """the shortest route along a corridor from its first voxel: every voxel under 6 neighbours; under 26 the voxels at which
    it turns are cut by a diagonal step (runs are 2 voxels or longer, so the two voxels around a turn are neighbours by an
    edge and no other pair is)"""
    voxels, turn = path
    return voxels if connectivity == 6 else voxels[~turn]


def s_path(y0, z, b=None, end=None):
    """a run along x from (0, y0, z) to x = 255, two voxels over in y, back to x = b, two over again and on to x = end > b
    (b=None: one run; end=None: two).  Seeded at its first voxel.  Every path reaches the volume's far face -- 15 tiles from
    its seed -- before it comes back, which is what keeps the sweeps above the first three batches."""
    corners = [(0, y0, z), (255, y0, z)]
    if b is not None:
        corners += [(255, y0 + 2, z), (b, y0 + 2, z)]
    if end is not None:
        corners += [(b, y0 + 4, z), (end, y0 + 4, z)]
    return polyline(corners)


class Scene:
    """name, depth, vol and seeds (uint8 [x, y, z]), through_empty, connectivities; quarter: where the farthest voxel is meant
    to fall (x / 64), or None; paths: the corridors as polyline()s, or None; waypoints(connectivity): voxels every chain from
    the seed to the last voxel reached passes in order, for a scene without corridors"""

    def __init__(self, name, depth, through_empty=False, quarter=None):
        self.name, self.depth, self.S, self.through_empty, self.quarter = name, depth, 1 << depth, through_empty, quarter
        self.vol = np.zeros((self.S,) * 3, np.uint8)
        self.seeds = np.zeros((self.S,) * 3, np.uint8)
        self.connectivities = (6, 26)
        self.paths = None
        self.waypoints = None

    def add_path(self, path, seeded=True):
        voxels = path[0]
        near = flood_model.dilate(self.vol != 0, 26)
        assert not near[tuple(voxels.T)].any(), "corridors must not touch, by corners either"
        self.vol[tuple(voxels.T)] = 1
        if seeded:
            self.seeds[tuple(voxels[0])] = 1
        self.paths = (self.paths or []) + [path]

    def freeze(self):
        self.vol.setflags(write=False)
        self.seeds.setflags(write=False)
        return self

    def forced_crossings(self, connectivity):
        """tile changes that some voxel's shortest chain from a seed cannot avoid: along the longest corridor's route, or
        from waypoint to waypoint"""
        if self.paths is not None:
            return max(crossings(route_of(p, connectivity), self.S) for p in self.paths)
        points = self.waypoints(connectivity)
        return sum(tile_distance(a, b, connectivity) for a, b in zip(points, points[1:]))

    def sweeps_implied(self, connectivity):
        """The sweeps of the schedule in which every tile of a sweep stages what the sweep before left (all tiles resident and
        staged together; one of the schedules the kernel must be right under): a value crosses a tile border only from one
        sweep to the next, so a voxel whose chain changes tile c times is final in sweep c + 1 at the earliest, and one more
        sweep counts 0.  A tile that stages a neighbour's stores of the same sweep can save sweeps, so the device may issue
        fewer: the GPU tests print its count and hold it only from above (max T + 2)."""
        return self.forced_crossings(connectivity) + 2


# ---- the scenes ---------------------------------------------------------------------------------------------------------

QUARTER_ENDS = (20, 84, 148, 212)            # x of the far end of the long corridor's second run, one per quarter


def quarters(k):
    """Four straight corridors along x in solid voxels.  A: (0..255, 37, 101), seeded at x = 0, joined at x = 255 by one voxel
    to B: (255 down to QUARTER_ENDS[k], 39, 101), whose end is the farthest voxel, 257 + 255 - end steps away, in the quarter
    [64 k, 64 k + 64) of x -- a dense index below 2^22 j is x < 64 j, so that is a lane's (k + 1)th quad in k_travel_stats.
    C: (30..99, 80, 15) seeded at x = 30 and D: (150..249, 120, 16) seeded at x = 249 are short, lie in other tiles and make
    the number of reached voxels different in every quarter."""
    s = Scene("quarters_%d" % k, 8, quarter=k)
    s.add_path(s_path(37, 101, QUARTER_ENDS[k]))
    s.add_path(polyline([(30, 80, 15), (99, 80, 15)]))
    s.add_path(polyline([(249, 120, 16), (150, 120, 16)]))
    return s.freeze()


# (y0, z, b, end): end - 2 b = 60, so every path is 574 steps long (570 under 26 neighbours: a turn saves two)
TIE_PATHS = {"q1": (20, 15, 10, 80), "q2": (60, 16, 40, 140), "q3": (100, 200, 70, 200),
             # the chosen pair: both ends in workgroup 16 * 64 + 10 of the stats pass, the winner (the smaller index) seen by
             # thread 255 in its second quad, the loser by thread 0 in its third
             "high_lane": (39, 253, 10, 80), "low_lane": (36, 2, 42, 144)}
TIES = {"two": ("q2", "q3"), "three": ("q1", "q2", "q3"), "lanes": ("high_lane", "low_lane")}


def ties(which):
    """Two or three corridors of equal length whose ends lie in different quarters of x: the smallest dense index must win,
    whichever iteration or lane sees it.  The winners lie beyond the first quarter, so that a loop without later iterations
    loses them.  "lanes": a smaller index is never seen in a LATER iteration than a larger one (qi = index / 4 is monotone in
    the index, vrc_travel.hip:231-237), so the pair that can tell a tie broken by who saw it from one broken by the index is
    the winner under the HIGHEST thread of a workgroup in an earlier iteration and the loser under thread 0 of the same
    workgroup in a later one: a combine that prefers the lower thread takes the loser."""
    s = Scene("ties_" + which, 8, quarter=min(TIE_PATHS[n][3] for n in TIES[which]) // 64)
    for n in TIES[which]:
        y0, z, b, end = TIE_PATHS[n]
        assert end - 2 * b == 60
        s.add_path(s_path(y0, z, b, end))
    return s.freeze()


SLAB_SEEDS = {"corner": (0, 0, 126), "interior": (21, 37, 129)}


def slab(where):
    """A slab 4 voxels thick in z across the whole x-y plane and one 4 thick in x across the whole y-z plane, both astride the
    tile border at 128 (travel's and the flood's): 520192 solid voxels in 960 travel tiles, the frontier crossing tile
    borders in all three axes.  One seed: the slab's corner, or a voxel inside it one tile in from the corner -- far enough
    from the far faces that 14 or more tile borders lie between under 26 neighbours as well."""
    s = Scene("slab_" + where, 8)
    s.vol[:, :, 126:130] = 1
    s.vol[126:130, :, :] = 1
    seed = SLAB_SEEDS[where]
    s.seeds[seed] = 1
    s.waypoints = lambda connectivity: [seed, (255, 255, 126)]
    return s.freeze()


SERPENTINES = {"rows": (80, 0, 255, 127), "corners": (105, 31, 224, 128)}          # rows, first y, last y, z


def serpentine(which):
    """A one-voxel corridor through one z layer: rows along y at x = 0, 2, 4, ..., joined at alternating ends, seeded at
    (0, first y, z).  "rows": 80 rows of 256, 20558 steps (20400 under 26 neighbours), 15 tile borders a row.  "corners": 105
    rows from y = 31 to y = 224, 20473 steps (20265), so that every turn lies on a tile border in y of both kernels (31 | 32
    and 223 | 224) and those at x = 15, 31, 47, ... on a corner of travel tiles, every second of them (x = 31 | 32 mod 32) on a
    corner of flood tiles too: there the diagonal step of 26 neighbours, (30, 32) -> (31, 31) -> (32, 32), goes through three
    tiles that meet at the corner.  (A flood tile is 32 voxels wide, so its borders lie at 31 | 32 mod 32.)"""
    rows, ya, yb, z = SERPENTINES[which]
    s = Scene("serpentine_" + which, 8)
    corners = []
    for i in range(rows):
        ends = (ya, yb) if i % 2 == 0 else (yb, ya)
        corners += [(2 * i, ends[0], z), (2 * i, ends[1], z)]
    s.add_path(polyline(corners))
    return s.freeze()


AIR_WALLS = ((37, (127, 127)), (70, (0, 0)), (101, (127, 0)))          # x of a full wall, (y, z) of its one-voxel door


def air128():
    """128^3, through the empty voxels: three full walls across x with one-voxel doors in alternating corners, one seed in the
    corner (0, 0, 0).  The dense case: 2 M voxels reached, all 512 travel tiles active."""
    s = Scene("air128", 7, through_empty=True)
    for x, (y, z) in AIR_WALLS:
        s.vol[x] = 1
        s.vol[x, y, z] = 0
    s.seeds[0, 0, 0] = 1
    s.waypoints = lambda connectivity: [(0, 0, 0)] + [(x, y, z) for x, (y, z) in AIR_WALLS] + [(127, 0, 127)]
    return s.freeze()


BUILDERS = {**{"quarters_%d" % k: functools.partial(quarters, k) for k in range(4)},
            **{"ties_" + w: functools.partial(ties, w) for w in TIES},
            **{"slab_" + w: functools.partial(slab, w) for w in SLAB_SEEDS},
            **{"serpentine_" + w: functools.partial(serpentine, w) for w in SERPENTINES},
            "air128": air128}
NAMES = list(BUILDERS)
CASES = [(name, connectivity) for name in NAMES for connectivity in (6, 26)]
LARGE = [name for name in NAMES if name != "air128"]          # the scenes at 256^3


@functools.lru_cache(maxsize=4)
def scene(name):
    """Shared by the tests: do not write to it."""
    return BUILDERS[name]()


class Sparse:
    """a field kept as (dense indices, values) of the voxels with a value"""

    def __init__(self, T):
        self.shape = T.shape
        flat = T.reshape(-1)
        self.idx = np.flatnonzero(flat != NONE)
        self.val = flat[self.idx].copy()

    def dense(self):
        T = np.full(self.shape, NONE, np.uint32)
        T.reshape(-1)[self.idx] = self.val
        return T


@functools.lru_cache(maxsize=None)
def _expected(name, connectivity):
    s = scene(name)
    return Sparse(travel_model.field(s.vol, s.seeds, connectivity, s.through_empty))


def expected_field(name, connectivity):
    """travel_model.field of the scene, dense; made once per scene and connectivity"""
    return _expected(name, connectivity).dense()


@functools.lru_cache(maxsize=None)
def _flooded(name, connectivity):
    s = scene(name)
    return np.flatnonzero(flood_model.flood(s.vol, s.seeds, connectivity, s.through_empty).reshape(-1))


def expected_region(name, connectivity):
    """flood_model.flood of the scene from the same seeds, dense uint8; made once per scene and connectivity"""
    s = scene(name)
    R = np.zeros((s.S,) * 3, np.uint8)
    R.reshape(-1)[_flooded(name, connectivity)] = 1
    return R


def n_seeds(name):
    s = scene(name)
    return int(travel_model.seeds_in_m(s.vol, s.seeds, s.through_empty).sum())


def far_end(name):
    """the last voxel of the serpentine's corridor"""
    return tuple(int(v) for v in scene(name).paths[0][0][-1])


@functools.lru_cache(maxsize=None)
def expected_route(name, connectivity):
    """travel_model.trace from the far end of a serpentine: (length, (length + 1, 3) route)"""
    return travel_model.trace(expected_field(name, connectivity), far_end(name), connectivity)


def sample_coordinates(T, seed):
    """4096 seeded voxels -- half of them among those with a value, the scenes being sparse -- and the 8 corners of the volume"""
    S = T.shape[0]
    rng = np.random.default_rng(seed)
    e = S - 1
    corners = [(x, y, z) for x in (0, e) for y in (0, e) for z in (0, e)]
    reached = np.flatnonzero(T.reshape(-1) != NONE)
    some = np.stack(np.unravel_index(reached[rng.integers(0, len(reached), 2048)], T.shape), axis=1)
    return np.concatenate([some, rng.integers(0, S, (2048, 3)), np.array(corners)]).astype(np.uint32)
