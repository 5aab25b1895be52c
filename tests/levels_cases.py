"""The cases of tests/test_gpu_volume_levels_large.py: volumes of 512^3 and 1024^3, where the launches of csrc/vrc_levels.hip
reach their cap of MAX_GROUPS workgroups and a lane (a workgroup, for k_counts_large) takes a SECOND item by grid stride.
Three things, numpy and Python integers only:
  the launch geometry of levels_counts_run, levels_reduce_run and levels_expand_run restated from the code as it stands
      (launches): per launch the kernel, the items, the items of one pass, the trips, and the maps between an item and
      the voxels it covers, so that the host test (tests/test_levels_cases_host.py) can hold the cases to the trips they
      are meant for;
  content as a list of solid coordinates (content): thin slabs of random points on both sides of every multiple of 64
      in x -- every trip seam of every launch lies on one --, the voxels on either side of each seam in the order of the
      items, the two corners of the volume, and a few aligned solid cubes;
  the models of the three calls on such a list, without an S^3 array (counts_sparse, counts_dense, reduce, expanded),
      held to levels_model.py on small dense volumes by the host test."""
import functools

import numpy as np

import levels_model
from levels_model import ANDNOT, OR, REPLACE  # noqa: F401

MAX_GROUPS = 16384                   # vrc_levels.hip: constexpr uint32_t MAX_GROUPS
GROUP = 256                          # lanes per workgroup of every launch there
LEVELS_GROUP_WORDS = 2048            # vrc_levels.h: the words of a cell that one workgroup sums


# ---- the layout: words of 2 x 2 x 8 voxels, cells of 2^k voxels per axis ----------------------------------------------

def word_of(p, depth):
    """the occupancy word of voxel p in a volume of depth >= 3: W = (cx * n + cy) * (n / 4) + wz (the top of vrc_levels.hip)"""
    n = 1 << (depth - 1)
    return ((p[:, 0] >> 1) * n + (p[:, 1] >> 1)) * (n >> 2) + (p[:, 2] >> 3)


def word_box(W, depth):
    n = 1 << (depth - 1)
    nz = n >> 2
    lo = np.stack([2 * (W // (nz * n)), 2 * ((W // nz) % n), 8 * (W % nz)], axis=1)
    return lo, lo + (2, 2, 8)


def voxel_item_of(P, depth):
    """k_reduce_voxels: lane i is bit i & 31 of word i >> 5; in 4^3 word cx, half cy"""
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    if depth == 2:
        return (X >> 1) * 32 + (Y >> 1) * 16 + Z * 4 + (Y & 1) * 2 + (X & 1)
    return word_of(P, depth) * 32 + (Z & 7) * 4 + (Y & 1) * 2 + (X & 1)


def voxel_item_box(i, depth):
    W, bit = i >> 5, i & 31
    if depth == 2:
        lo = np.stack([2 * W + (bit & 1), 2 * (bit >> 4) + ((bit >> 1) & 1), (bit >> 2) & 3], axis=1)
    else:
        lo, _ = word_box(W, depth)
        lo = lo + np.stack([bit & 1, (bit >> 1) & 1, bit >> 2], axis=1)
    return lo, lo + 1


def cell_of(p, depth, k):
    """the dense index (X * Sc + Y) * Sc + Z of the cell of level k that holds voxel p"""
    Sc = 1 << (depth - k)
    q = p >> k
    return (q[:, 0] * Sc + q[:, 1]) * Sc + q[:, 2]


def cell_box(c, depth, k):
    Sc = 1 << (depth - k)
    lo = np.stack([c // (Sc * Sc), (c // Sc) % Sc, c % Sc], axis=1) << k
    return lo, lo + (1 << k)


# ---- the launches ---------------------------------------------------------------------------------------------------

class Launch:
    """kernel; items; per_pass (items the whole grid takes in one trip of its loop); trips; space ("src" or "dst") and
    depth of the volume whose voxels the items cover; item_of((n, 3) int64 voxels of that volume) -> items; cover(items) ->
    (lo, hi), the box of voxels of that volume that an item reads (src) or writes (dst)"""

    def __init__(self, kernel, items, per_pass, space, depth, item_of, cover):
        self.kernel, self.items, self.per_pass, self.space, self.depth = kernel, items, per_pass, space, depth
        self.trips = -(-items // per_pass)
        self.item_of, self.cover = item_of, cover

    def seams(self):
        """the first item of every trip after the first"""
        return [t * self.per_pass for t in range(1, self.trips)]

    def row(self):
        return (self.kernel, self.items, self.per_pass, self.trips)


def groups_for(lanes):
    """vrc_levels.hip, groups_for"""
    return min((lanes + GROUP - 1) // GROUP, MAX_GROUPS)


def per_lane(kernel, items, space, depth, item_of, cover):
    return Launch(kernel, items, groups_for(items) * GROUP, space, depth, item_of, cover)


def counts_launch(depth, k):
    """levels_counts_run"""
    lgs, lc = depth - 1, depth - k
    if k == 1:
        return per_lane("k_counts_bytes", 1 << (3 * lgs - 2), "src", depth, lambda p: word_of(p, depth), lambda W: word_box(W, depth))
    if k in (2, 3):
        return per_lane("k_counts_small<%d>" % k, 1 << (3 * lc), "src", depth, lambda p: cell_of(p, depth, k), lambda c: cell_box(c, depth, k))
    # k_counts_large: unit u = (cell, part), a workgroup per unit; a part is LEVELS_GROUP_WORDS words of the cell's
    # 2^(3 lgc - 2), numbered along the cell's brick rows: word `it` is word it & (c / 4 - 1) of row it >> lgw, row r is
    # brick row (r >> lgc, r & (c - 1)) of the cell
    lgp = max(3 * k - 16, 0)
    lgc = k - 1
    lgw = lgc - 2
    units = 1 << (3 * lc + lgp)
    c = 1 << lgc
    part_rows = min(LEVELS_GROUP_WORDS >> lgw, c * c)

    def item_of(p):
        b = (p >> 1) & (c - 1)
        it = ((b[:, 0] * c + b[:, 1]) << lgw) | (b[:, 2] >> 2)
        return (cell_of(p, depth, k) << lgp) | (it // LEVELS_GROUP_WORDS)

    def cover(u):
        lo, hi = cell_box(u >> lgp, depth, k)
        r0 = (u & ((1 << lgp) - 1)) * part_rows
        lo, hi = lo.copy(), hi.copy()
        lo[:, 0] += 2 * (r0 >> lgc)
        if part_rows >= c:
            hi[:, 0] = lo[:, 0] + 2 * (part_rows >> lgc)
        else:
            hi[:, 0] = lo[:, 0] + 2
            lo[:, 1] += 2 * (r0 & (c - 1))
            hi[:, 1] = lo[:, 1] + 2 * part_rows
        return lo, hi

    return Launch("k_counts_large", units, min(units, MAX_GROUPS), "src", depth, item_of, cover)


def launches(kind, src_depth, k):
    """the kernels of one call in the order of their launches.  kind: "counts" (cellCounts(k) of a volume of src_depth),
    "reduce" (into depth src_depth - k) or "expand" (into depth src_depth + k)"""
    if kind == "counts":
        return [counts_launch(src_depth, k)]
    if kind == "expand":
        d = src_depth + k
        return [per_lane("k_expand", 1 << (3 * (d - 1) - 2), "dst", d, lambda p: word_of(p, d), lambda W: word_box(W, d))]
    d = src_depth - k                                                        # levels_reduce_run
    lgd = d - 1
    if k == 1 and lgd >= 2:
        return [per_lane("k_reduce_bytes", 1 << (3 * lgd - 2), "dst", d, lambda p: word_of(p, d), lambda W: word_box(W, d))]
    voxels = per_lane("k_reduce_voxels<%d>" % (k if k < 4 else 0), 8 << (3 * lgd), "dst", d, lambda p: voxel_item_of(p, d), lambda i: voxel_item_box(i, d))
    return [voxels] if k < 4 else [counts_launch(src_depth, k), voxels]


def striding(kind, src_depth, k):
    """the one launch of the call that the cases are about: the first that takes more than one trip, else the first"""
    ls = launches(kind, src_depth, k)
    return next((l for l in ls if l.trips > 1), ls[0])


def item_facts(launch, items, values=None):
    """what the host test asks of the sorted, unique items with non-zero expected output (values: their outputs, where
    the bare set of items is not the whole output): the trips that hold one, whether item 0 and the last item are among
    them, the seams with such an item on both sides, and whether the trips' outputs, each moved back to trip 0, differ
    from one another"""
    items = np.asarray(items, np.int64)
    assert len(items) and (np.diff(items) > 0).all() and 0 <= items[0] and items[-1] < launch.items
    values = np.ones(len(items), np.int64) if values is None else np.asarray(values, np.int64)
    trip = items // launch.per_pass
    seams = np.array(launch.seams(), np.int64)
    both = np.isin(seams - 1, items) & np.isin(seams, items)
    images = {(items[trip == t] - t * launch.per_pass).tobytes() + values[trip == t].tobytes() for t in range(launch.trips)}
    return {"trips": sorted(set(trip.tolist())), "first": int(items[0]) == 0, "last": int(items[-1]) == launch.items - 1,
            "seams": seams[both].tolist(), "distinct": len(images) == launch.trips}


# ---- content ----------------------------------------------------------------------------------------------------------

# depth: (the pitch of the slabs in x, random points per slab, [(side, low corner)] of the aligned solid cubes).  Depths 9
# and 10 are sources of counts and reduce (seams at multiples of 64) and depth 9 of the expansion into depth 10 (k_expand's
# seams every 128 of the destination's x); depth 7 is expanded into depth 10 with k = 3, every 16 of its x
CONTENT = {
    10: (64, 12000, [(64, (448, 512, 256)), (32, (96, 32, 992)), (32, (800, 960, 0)), (16, (1008, 1008, 16)), (16, (16, 496, 512))]),
    9: (64, 8000, [(32, (224, 64, 480)), (16, (288, 496, 0)), (16, (48, 0, 496))]),
    7: (16, 100, [(4, (60, 64, 0))]),
}


class Content:
    """points (n, 3) uint32 for setVoxels and boxes (m, 6) uint32 for fillBoxes: the upload; solid (N, 3) int64: every solid
    voxel once, in the order of the voxel list (list_key)"""


@functools.lru_cache(maxsize=None)
def content(depth, seed=2024):
    """Shared by the tests: do not write to it."""
    pitch, per_slab, cubes = CONTENT[depth]
    S = 1 << depth
    rng = np.random.default_rng(seed + depth)
    parts = [np.array([(0, 0, 0), (S - 1, S - 1, S - 1)], np.int64)]
    for s in range(pitch, S, pitch):
        x = s + rng.integers(-2, 2, per_slab)
        wide = rng.integers(0, S, (per_slab, 2))
        wide[per_slab // 2:] >>= 3                                            # half of them in 1/64 of the slab: cells of every count
        parts += [np.column_stack([x, wide]), np.array([(s, 0, 0), (s - 1, S - 1, S - 1)], np.int64)]
    c = Content()
    c.depth = depth
    c.points = in_list_order(np.concatenate(parts), depth).astype(np.uint32)
    c.boxes = np.array([list(lo) + [v + side for v in lo] for side, lo in cubes], np.uint32)
    assert all(v % side == 0 for side, lo in cubes for v in lo)
    filled = [np.indices((side,) * 3).reshape(3, -1).T + np.array(lo, np.int64) for side, lo in cubes]
    c.solid = in_list_order(np.concatenate([c.points.astype(np.int64)] + filled), depth)
    for a in (c.points, c.boxes, c.solid):
        a.setflags(write=False)
    return c


def upload(volume, c):
    volume.setVoxels(c.points)
    volume.fillBoxes(c.boxes)
    return volume


# ---- the models on a list of solid voxels -----------------------------------------------------------------------------------

def list_key(p, depth):
    """include/vrc.h, the order of vrc_voxels_extract: 8 B + (z & 1) 4 + (y & 1) 2 + (x & 1), B the brick index"""
    n = 1 << (depth - 1)
    return 8 * (((p[:, 0] >> 1) * n + (p[:, 1] >> 1)) * n + (p[:, 2] >> 1)) + (p[:, 2] & 1) * 4 + (p[:, 1] & 1) * 2 + (p[:, 0] & 1)


def in_list_order(p, depth):
    """the distinct voxels of p (n, 3), int64, ascending by list_key"""
    p = np.asarray(p, np.int64).reshape(-1, 3)
    _, first = np.unique(list_key(p, depth), return_index=True)
    return p[first]


def counts_sparse(solid, depth, k):
    """(the dense indices of the non-empty cells of level k, ascending; their counts)"""
    return np.unique(cell_of(np.asarray(solid, np.int64), depth, k), return_counts=True)


def counts_dense(solid, depth, k):
    """levels_model.counts of the volume that holds `solid`, for (S >> k)^3 that fits the host"""
    Sc = 1 << (depth - k)
    cells, c = counts_sparse(solid, depth, k)
    out = np.zeros(Sc ** 3, np.uint32)
    out[cells] = c
    return out.reshape(Sc, Sc, Sc)


def reduce(dst, solid, depth, lo, hi, op=REPLACE):
    """levels_model.reduce: a copy of the dense dst after reduceInto from the volume of `depth` that holds `solid`"""
    k = depth - (dst.shape[0].bit_length() - 1)
    c = counts_dense(solid, depth, k).astype(np.int64)
    return levels_model.apply_op(dst.astype(np.uint8), ((c >= lo) & (c < hi)).astype(np.uint8), op)


def selected(solid, depth, k, lo, hi):
    """the voxels of the destination that a band with lo >= 1 selects, (n, 3) int64"""
    assert lo >= 1
    cells, c = counts_sparse(solid, depth, k)
    lo_corner, _ = cell_box(cells[(c >= lo) & (c < hi)], depth, k)
    return lo_corner >> k


def expanded(solid, k):
    """the solid voxels of the volume of depth + k after expandInto with REPLACE: every voxel times its 2^k cube"""
    cube = np.indices((1 << k,) * 3).reshape(3, -1).T
    return ((np.asarray(solid, np.int64)[:, None, :] << k) + cube[None]).reshape(-1, 3)


def dense_of(solid, depth):
    vol = np.zeros((1 << depth,) * 3, np.uint8)
    vol[tuple(np.asarray(solid, np.int64).T)] = 1
    return vol


def split_band(solid, depth, k):
    """(lo, 8^k + 1) with lo the median count of the non-empty cells, one more where that is the smallest count: a band
    chosen from the content alone.  That it selects some and not all of them is the host test's to assert"""
    _, c = counts_sparse(solid, depth, k)
    lo = int(np.median(c))
    return (lo + 1 if lo == int(c.min()) else lo), 8 ** k + 1


# ---- the calls of tests/test_gpu_volume_levels_large.py -------------------------------------------------------------------------

# (kind, source depth, k): every call of the GPU tests; CASES is what the summary's trip table is printed from
CASES = [("counts", 9, 4), ("counts", 9, 5), ("counts", 9, 9), ("reduce", 9, 4),
         ("counts", 10, 1), ("counts", 10, 2), ("counts", 10, 4), ("counts", 10, 5), ("counts", 10, 6), ("counts", 10, 10),
         ("reduce", 10, 2), ("reduce", 10, 4), ("reduce", 10, 5), ("reduce", 10, 6),
         ("expand", 9, 1), ("expand", 7, 3)]


def nonzero_items(kind, src_depth, k, band=None):
    """(the launch of the call that strides, the sorted items of it whose expected output is not zero, their outputs or
    None) under content(src_depth): counts of the items of a counts kernel, the selected voxels of k_reduce_voxels under
    `band` ("any" where None), the words of k_expand that hold a solid voxel"""
    launch = striding(kind, src_depth, k)
    solid = content(src_depth).solid
    if launch.kernel.startswith("k_counts"):
        items, values = np.unique(launch.item_of(solid), return_counts=True)
        return launch, items, values
    if kind == "expand":
        return launch, np.unique(launch.item_of(expanded(solid, k))), None
    lo, hi = band or levels_model.count_range("any", k)
    return launch, np.unique(launch.item_of(selected(solid, src_depth, k, lo, hi))), None


def trip_table():
    return [(kind, depth, k) + l.row() for kind, depth, k in CASES for l in launches(kind, depth, k)]
