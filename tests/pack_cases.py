"""The cases of tests/test_gpu_volume_pack_large.py: volumes at which the kernels of csrc/vrc_pack.hip leave the regime the
smaller tests keep them in.  Three things, numpy and Python integers only:
  the launch geometry of the pack and unpack passes restated from the code as it stands, each with the function it was
      read from, so that the host test (tests/test_pack_cases_host.py) can hold the cases to the trips, steps and ranks
      they are meant for;
  three volumes as lists of edits (large_volume_cases.dense_of's form) with the brick bytes the same list gives in numpy
      -- no dense array: a 1024^3 one is 1 GiB, its bricks are 128 MiB -- and pack_model's stream of those bricks:
      strided_512 (k_unpack_bytes takes three trips), all_mixed_256 (every tile mixed, ranks and offsets large),
      sparse_1024 (depth 10: row_of<true> with lgt = 6, 256 scan steps);
  corruptions of the first two streams at chosen tiles and bytes, with the (rule, where) pack_model.unpack_bricks gives
      for each."""
import functools
import struct

import numpy as np

import pack_model as model
from large_volume_cases import SCAN_GROUP, plane_boxes, scan_steps  # noqa: F401  (vrc_group.h, restated once)

GROUP = 256                          # lanes per workgroup of k_pack_head, k_unpack_classes, k_unpack_masks, k_unpack_bytes
BYTE_GROUPS = 4096                   # vrc_pack.hip, unpack_check_run: if (groups > 4096u) groups = 4096u


# ---- the launch geometry ----------------------------------------------------------------------------------------------

def pack_tiles(depth):
    """vrc_pack.h, pack_tiles: (pack_n / pack_edge)^3 with pack_n = 2^(depth - 1) and pack_edge = min(pack_n, 8)"""
    n = 1 << (depth - 1)
    return (n // min(n, 8)) ** 3


def pack_tile_bricks(depth):
    """vrc_pack.h, pack_tile_bricks"""
    return min(1 << (depth - 1), 8) ** 3


def pack_mask_words(depth):
    """vrc_pack.h, pack_mask_words: a mask of K bits in whole words, one word below 32 bits"""
    return max(1, pack_tile_bricks(depth) // 32)


def pack_class_words(depth):
    """vrc_pack.h, pack_class_words: 16 class fields a word"""
    return (pack_tiles(depth) + 15) // 16


def field_groups(depth):
    """vrc_pack.hip, field_groups: the workgroups of k_pack_head and k_unpack_classes, a lane per class field"""
    return (16 * pack_class_words(depth) + GROUP - 1) // GROUP


def mask_groups(depth):
    """vrc_pack.hip, unpack_check_run: the grid of k_unpack_masks, MW lanes per tile"""
    return (pack_tiles(depth) * pack_mask_words(depth) + GROUP - 1) // GROUP


def tile_groups(depth):
    """vrc_pack.hip, pack_offsets_run, pack_emit_run, unpack_write_run: one wave per tile"""
    return pack_tiles(depth)


def byte_words(P):
    """vrc_pack.hip, k_unpack_bytes: n_words = (P + 3) / 4"""
    return (P + 3) // 4


def byte_groups(P):
    """vrc_pack.hip, unpack_check_run: the workgroups of k_unpack_bytes, capped at 4096; no launch without a word"""
    return min((byte_words(P) + GROUP - 1) // GROUP, BYTE_GROUPS)


def byte_trips(P):
    """the most words a lane of k_unpack_bytes takes: for (i = lane; i < n_words; i += gridDim.x * 256)"""
    lanes = byte_groups(P) * GROUP
    return -(-byte_words(P) // lanes) if lanes else 0


def byte_trip_of(P, at):
    """the trip of that loop in which byte `at` of D (or of the padding behind it) is read"""
    return (at // 4) // (byte_groups(P) * GROUP)


def tile_number(depth, tx, ty, tz):
    """vrc.h: tile t = (tx T + ty) T + tz"""
    T = model.Shape(depth).T
    return (tx * T + ty) * T + tz


def tile_origin(depth, t):
    """the least voxel of tile t (row_of<true>: tx = t >> 2 lgt, ty = (t >> lgt) & (T - 1), tz = t & (T - 1))"""
    s = model.Shape(depth)
    return np.array([t // (s.T * s.T), (t // s.T) % s.T, t % s.T], np.int64) * (2 * s.E)


# ---- edits on brick bytes ---------------------------------------------------------------------------------------------

def bricks_of_edits(edits, depth):
    """pack_model.bricks_of(large_volume_cases.dense_of(edits, S)) without the dense array.  edits: [("boxes", (n, 6), solid) |
    ("voxels", (n, 3), solid)] applied in order, boxes clipped to the volume and voxels outside it dropped, as the device does"""
    S, n = 1 << depth, 1 << (depth - 1)
    bricks = np.zeros((n, n, n), np.uint8)
    for kind, items, solid in edits:
        items = np.asarray(items, np.int64)
        if kind == "boxes":
            for box in items:
                lo, hi = np.minimum(box[:3], S), np.minimum(box[3:], S)
                if (lo >= hi).any():
                    continue
                for bit in range(8):
                    off = (bit & 1, (bit >> 1) & 1, bit >> 2)
                    sl = tuple(slice(int(lo[a] - off[a] + 1) // 2, int(hi[a] - off[a] + 1) // 2) for a in range(3))
                    if solid:
                        bricks[sl] |= np.uint8(1 << bit)
                    else:
                        bricks[sl] &= np.uint8(0xFF ^ (1 << bit))
        elif kind == "voxels":
            items = items[((items >= 0) & (items < S)).all(1)]
            at = tuple((items >> 1).T)
            bits = (1 << ((items[:, 2] & 1) * 4 + (items[:, 1] & 1) * 2 + (items[:, 0] & 1))).astype(np.uint8)
            if solid:
                np.bitwise_or.at(bricks, at, bits)
            else:
                np.bitwise_and.at(bricks, at, np.uint8(0xFF) ^ bits)
        else:
            raise ValueError(kind)
    return bricks


def upload(volume, edits):
    """the same list on the device"""
    for kind, items, solid in edits:
        (volume.fillBoxes if kind == "boxes" else volume.setVoxels)(np.asarray(items, np.uint32), bool(solid))
    return volume


def solid_at(bricks, xyz):
    """uint8 0 / 1 per (n, 3) voxel coordinate, 0 outside the volume: VoxelVolume.getVoxels"""
    xyz = np.asarray(xyz, np.int64)
    inside = ((xyz >= 0) & (xyz < 2 * bricks.shape[0])).all(1)
    p = xyz[inside]
    out = np.zeros(len(xyz), np.uint8)
    out[inside] = (bricks[tuple((p >> 1).T)] >> ((p[:, 2] & 1) * 4 + (p[:, 1] & 1) * 2 + (p[:, 0] & 1))) & 1
    return out


def voxels_of(bricks):
    """(n, 3) uint32: the solid voxels, setVoxels' input"""
    return np.argwhere(model.dense_of(bricks)).astype(np.uint32)


class Case:
    """name, depth, edits (the upload), bricks [cx, cy, cz] (read-only), stream (pack_model's bytes), header (its 16 words)"""

    def __init__(self, name, depth, edits, bricks):
        bricks.setflags(write=False)
        self.name, self.depth, self.edits, self.bricks = name, depth, edits, bricks
        self.stream = model.pack_bricks(bricks, depth)
        self.header = model.header_of(self.stream)
        self.M, self.P, self.full = self.header[4], self.header[5], self.header[10]
        self.solid = self.header[8] | (self.header[9] << 32)

    def partial_counts(self):
        """section B: the partial bricks of each mixed tile, by rank"""
        s = model.Shape(self.depth)
        return np.frombuffer(self.stream, "<u4", self.M, s.offsets(self.M, self.P)[1]).astype(np.int64)

    def classes(self):
        s = model.Shape(self.depth)
        A = np.frombuffer(self.stream, "<u4", s.CW, 64)
        return ((A[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)[:s.NT]


# ---- A. strided_512 ----------------------------------------------------------------------------------------------------

A_FULL = [[32, 48, 64, 64, 64, 96]]                                            # 2 x 1 x 2 whole tiles
A_EMPTY = [[256, 32, 64, 288, 48, 96], [496, 496, 480, 512, 512, 496]]         # 2 x 1 x 2 tiles, and tile 32766
A_LONE = [[257, 33, 65], [260, 35, 69], [263, 41, 66], [270, 46, 77]]             # single voxels in the first emptied tile: they set P % 4


def strided_edits(extra=None):
    """512^3: slabs one voxel thick at every fifth z and every fifth y, so that a brick is empty only where neither of its two
    z nor of its two y is a multiple of five -- (3/5)^2 of them: about 64 % of 2^24 bricks are partial, 10.7 million, more than
    twice 2^22 --, 300000 voxels set and 100000 cleared at seeded places, a box of whole tiles filled and two cleared"""
    rng = np.random.default_rng(5120)
    edits = [("boxes", plane_boxes(512, 2, 5), 1), ("boxes", plane_boxes(512, 1, 5), 1),
             ("voxels", rng.integers(0, 512, (300000, 3)).astype(np.uint32), 1), ("voxels", rng.integers(0, 512, (100000, 3)).astype(np.uint32), 0),
             ("boxes", np.array(A_FULL, np.uint32), 1), ("boxes", np.array(A_EMPTY, np.uint32), 0), ("voxels", np.array(A_LONE, np.uint32), 1)]
    return edits + ([("voxels", extra, 1)] if extra is not None else [])


@functools.lru_cache(maxsize=None)
def strided_512():
    """Shared by the tests: do not write to it."""
    edits = strided_edits()
    return Case("strided_512", 9, edits, bricks_of_edits(edits, 9))


@functools.lru_cache(maxsize=None)
def ordering_case():
    """(extra, stream): 200000 seeded voxels (n, 3) uint32 set behind strided_512's content, and the model's stream of the
    edited bricks"""
    extra = np.random.default_rng(5121).integers(0, 512, (200000, 3)).astype(np.uint32)
    bricks = strided_512().bricks.copy()
    at = tuple((extra.astype(np.int64) >> 1).T)
    np.bitwise_or.at(bricks, at, (1 << ((extra[:, 2] & 1) * 4 + (extra[:, 1] & 1) * 2 + (extra[:, 0] & 1))).astype(np.uint8))
    return extra, model.pack_bricks(bricks, 9)


# ---- B. all_mixed_256 --------------------------------------------------------------------------------------------------

B_HIGH = range(0, 1024)              # the run of tiles with 500 or more partial bricks: the first scan step


def all_mixed_counts():
    """the partial bricks of each of the 4096 tiles: 500 + (5 t mod 13) over the first 1024 tiles (500..512, 512 where
    5 t = 12 mod 13), seeded draws from 1..499 behind them, 1 in tiles 1024 and 4095"""
    rng = np.random.default_rng(256)
    t = np.arange(4096)
    counts = rng.integers(1, 500, 4096)
    counts[B_HIGH] = 500 + (5 * t[B_HIGH]) % 13
    counts[[1024, 4095]] = 1
    return counts


@functools.lru_cache(maxsize=None)
def all_mixed_256():
    """256^3, every tile mixed.  Tile t holds counts[t] partial bricks at the local indices (a j + b) mod 512, j < counts[t],
    with a odd and b from t -- a permutation of the tile, another in every tile --, their bytes 1 + (37 q + 11 t) mod 254
    (never 0x00 or 0xff), and one full brick at index j = counts[t] where there is room.  Shared: do not write to it."""
    s = model.Shape(8)
    counts = all_mixed_counts()
    t = np.arange(s.NT, dtype=np.int64)[:, None]
    j = np.arange(s.K, dtype=np.int64)[None, :]
    q = ((2 * (t % 97) + 1) * j + 7 * t) % s.K
    value = np.where(j < counts[:, None], 1 + (37 * q + 11 * t) % 254, np.where(j == counts[:, None], 0xFF, 0)).astype(np.uint8)
    tiles = np.zeros((s.NT, s.K), np.uint8)
    tiles[t, q] = value
    bricks = np.ascontiguousarray(model.bricks_from_tiles(tiles, s))
    return Case("all_mixed_256", 8, [("voxels", voxels_of(bricks), 1)], bricks)


# ---- C. sparse_1024 ----------------------------------------------------------------------------------------------------

C_BOUNDARY_STEPS = (1, 2, 100, 128, 255)                                       # tiles 1024 k - 1 and 1024 k; 255: the last boundary
C_FULL_BOXES = [[512, 256, 128, 544, 272, 176],                                # 2 x 1 x 3 whole tiles
                [16, 1008, 0, 32, 1024, 16],                                   # tile (1, 63, 0) = 8128
                [1000, 40, 600, 1024, 70, 640]]                                # aligned to nothing: whole tiles inside, mixed ones around


def sparse_listed_tiles():
    """tiles 0, 1 and 262143, both sides of the chosen step boundaries, the eight corner tiles"""
    corners = [tile_number(10, x, y, z) for x in (0, 63) for y in (0, 63) for z in (0, 63)]
    sides = [1024 * k + d for k in C_BOUNDARY_STEPS for d in (-1, 0)]
    return sorted(set([0, 1, 262143] + sides + corners))


def sparse_edits():
    """1024^3: the boxes above, 3000 single voxels and 200 boxes of up to 5 voxels a side at seeded places, and in the i-th
    listed tile i mod 7 + 1 voxels in bricks of their own plus the tile's far corner voxel"""
    rng = np.random.default_rng(1024)
    lo = rng.integers(0, 1020, (200, 3))
    small = np.concatenate([lo, lo + rng.integers(1, 6, (200, 3))], axis=1)
    placed = []
    for i, t in enumerate(sparse_listed_tiles()):
        o = tile_origin(10, t)
        placed += [o + (2 * m + (i & 1), 4 + ((i >> 1) & 1), 2 * ((m * 3 + i) % 8)) for m in range(i % 7 + 1)] + [o + 15]
    return [("boxes", np.array(C_FULL_BOXES, np.uint32), 1), ("voxels", rng.integers(0, 1024, (3000, 3)).astype(np.uint32), 1),
            ("boxes", small.astype(np.uint32), 1), ("voxels", np.array(placed, np.uint32), 1)]


@functools.lru_cache(maxsize=None)
def sparse_1024():
    """Shared by the tests: do not write to it."""
    edits = sparse_edits()
    return Case("sparse_1024", 10, edits, bricks_of_edits(edits, 10))


def sparse_places():
    """(n, 3) int64: every single voxel of the list and the corners of its boxes, each with its 26 neighbours -- some of
    them outside the volume, where getVoxels reads 0"""
    pts = []
    for kind, items, _ in sparse_edits():
        items = np.asarray(items, np.int64)
        pts.append(items if kind == "voxels" else np.concatenate([items[:, :3], items[:, 3:] - 1]))
    around = np.indices((3, 3, 3)).reshape(3, -1).T - 1
    return (np.concatenate(pts)[:, None, :] + around[None]).reshape(-1, 3)


CASES = {"strided_512": strided_512, "all_mixed_256": all_mixed_256, "sparse_1024": sparse_1024}


# ---- D. corruptions at chosen places -----------------------------------------------------------------------------------

def with_byte(stream, at, value):
    return stream[:at] + bytes([value]) + stream[at + 1:]


def with_class(stream, t, value):
    """class field t of section A"""
    at = 64 + 4 * (t // 16)
    word = struct.unpack_from("<I", stream, at)[0]
    return model.set_words(stream, at, (word & ~(3 << (2 * (t % 16)))) | (value << (2 * (t % 16))))


def with_tile_rule(stream, rule, t):
    """`stream` with `rule` broken in mixed tile t"""
    h = model.header_of(stream)
    s = model.Shape(h[2])
    _, b, c, _, _ = s.offsets(h[4], h[5])
    A = np.frombuffer(stream, "<u4", s.CW, 64)
    cls = ((A[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)[:s.NT]
    assert cls[t] == 2
    r = int((cls[:t] == 2).sum())
    if rule == "class-map":
        return with_class(stream, t, 3)
    if rule == "mixed-count":
        return with_class(stream, t, 0)
    if rule == "partial-count":
        return model.set_words(stream, b + 4 * r, struct.unpack_from("<I", stream, b + 4 * r)[0] + 1)
    at = c + 8 * s.MW * r
    w = struct.unpack_from("<%dI" % (2 * s.MW), stream, at)
    some, full = list(w[:s.MW]), list(w[s.MW:])
    if rule == "full-in-some":
        q = next((q for q in range(s.K) if not (some[q // 32] >> (q % 32)) & 1), None)       # an empty brick claimed full,
        if q is None:
            q = next(q for q in range(s.K) if not (full[q // 32] >> (q % 32)) & 1)           # failing that a partial one
        some[q // 32] &= ~(1 << (q % 32))
        full[q // 32] |= 1 << (q % 32)
    elif rule == "some-empty":
        some, full = [0] * s.MW, [0] * s.MW
    elif rule == "full-whole":
        some, full = [0xFFFFFFFF] * s.MW, [0xFFFFFFFF] * s.MW
    else:
        raise ValueError(rule)
    return model.set_words(stream, at, *some, *full)


def expectation(stream, depth):
    got = model.unpack_bricks(stream, depth)
    assert isinstance(got, tuple)
    return got


A_CORRUPTIONS = ["zero byte, trip 1", "zero byte, last trip", "ff byte, trip 1", "ff byte, last trip", "padding", "solid count",
                 "two bytes, trips 1 and 2", "byte and padding"]


def a_places():
    """byte indices into D of strided_512 that a lane of k_unpack_bytes reaches on trip 1 and on the last trip"""
    case = strided_512()
    lanes = byte_groups(case.P) * GROUP
    last = byte_trips(case.P) - 1
    return {"trip 1": 4 * (lanes + 12345) + 1, "trip 1 b": 4 * (2 * lanes - 1) + 3, "last": 4 * (last * lanes + 777) + 2, "last b": case.P - 2}


@functools.lru_cache(maxsize=None)
def a_corruption(name):
    """(bytes, rule, where) -- rule and where as pack_model.unpack_bricks names them"""
    case = strided_512()
    stream = case.stream
    d, length = model.Shape(9).offsets(case.M, case.P)[3:]
    at = a_places()
    if name == "zero byte, trip 1":
        bad = with_byte(stream, d + at["trip 1"], 0)
    elif name == "zero byte, last trip":
        bad = with_byte(stream, d + at["last"], 0)
    elif name == "ff byte, trip 1":
        bad = with_byte(stream, d + at["trip 1 b"], 0xFF)
    elif name == "ff byte, last trip":
        bad = with_byte(stream, d + at["last b"], 0xFF)
    elif name == "padding":
        bad = with_byte(stream, length - 1, 0x80)
    elif name == "solid count":                               # another legal byte with one voxel more or less, in the last trip
        v = stream[d + at["last"]]
        bad = with_byte(stream, d + at["last"], v ^ 1 if (v ^ 1) not in (0, 0xFF) else v ^ 2)
    elif name == "two bytes, trips 1 and 2":
        bad = with_byte(with_byte(stream, d + at["last"], 0xFF), d + at["trip 1"], 0)
    elif name == "byte and padding":
        bad = with_byte(with_byte(stream, length - 1, 1), d + at["last b"], 0)
    else:
        raise ValueError(name)
    return (bad,) + expectation(bad, 9)


B_TILES = (1023, 1024, 2500, 4095)
B_RULES = ["full-in-some", "some-empty", "full-whole", "partial-count", "class-map", "mixed-count"]
B_PAIRS = ((2500, 1024), (1023, 4095))                        # two tiles broken at once: the lower one is reported


@functools.lru_cache(maxsize=None)
def b_corruptions(rule):
    """[(tiles, bytes, rule, where)] of all_mixed_256's stream: `rule` broken in each of B_TILES alone and in each pair"""
    stream = all_mixed_256().stream
    out = []
    for tiles in [(t,) for t in B_TILES] + list(B_PAIRS):
        bad = stream
        for t in tiles:
            bad = with_tile_rule(bad, rule, t)
        out.append((tiles, bad) + expectation(bad, 8))
    return out


# ---- the byte check, restated -------------------------------------------------------------------------------------------

def byte_check(stream, words=None):
    """k_unpack_bytes over section D of a stream whose header holds, the loop cut after `words` words (None: all of them):
    (first_byte, first_padding, the solid voxels it adds) with None for a first_* that nothing sets"""
    h = model.header_of(stream)
    P = h[5]
    d = model.Shape(h[2]).offsets(h[4], P)[3]
    n = byte_words(P) if words is None else min(words, byte_words(P))
    D = np.frombuffer(stream, np.uint8, 4 * n, d)
    inside = D[:min(P, 4 * n)]
    bad = np.flatnonzero((inside == 0) | (inside == 0xFF))
    pad = np.flatnonzero(D[len(inside):] != 0)
    return (d + int(bad[0]) if len(bad) else None, d + len(inside) + int(pad[0]) if len(pad) else None, model.solid_of(inside))


def mask_solid(stream):
    """the solid voxels k_unpack_classes and k_unpack_masks account for: 8 K per full tile, 8 per bit of a full mask"""
    h = model.header_of(stream)
    s = model.Shape(h[2])
    c = s.offsets(h[4], h[5])[2]
    Cw = np.frombuffer(stream, "<u4", 2 * s.MW * h[4], c).reshape(h[4], 2, s.MW)
    full_bits = int(np.unpackbits(np.ascontiguousarray(Cw[:, 1]).view(np.uint8)).sum(dtype=np.int64))
    return 8 * s.K * h[10] + 8 * full_bits
