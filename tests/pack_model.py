"""The sparse tile stream of a volume (include/vrc.h: vrc_pack_*; format version 1) in numpy: pack, unpack with the
canonical rules in the header's order, and corrupt(), which breaks one rule of a valid stream at a time.  No GPU."""
import struct

import numpy as np

MAGIC, VERSION = 0x50435256, 1
HEADER_RULES = ["header-short", "magic-version", "depth", "tiles", "reserved", "length-argument", "length-formula", "count-limits"]
DEVICE_RULES = ["class-map", "mixed-count", "full-count", "full-in-some", "mask-range", "some-empty", "full-whole", "partial-count",
                "partial-sum", "partial-byte", "padding", "solid-count"]
RULES = HEADER_RULES + DEVICE_RULES
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


class Shape:
    def __init__(self, depth):
        self.depth = depth
        self.S = 1 << depth
        self.n = self.S // 2
        self.E = min(8, self.n)
        self.T = self.n // self.E
        self.NT = self.T ** 3
        self.K = self.E ** 3
        self.MW = max(1, self.K // 32)
        self.CW = (self.NT + 15) // 16

    def offsets(self, M, P):
        """the byte offsets of A, B, C, D and the length"""
        a = 64
        b = a + 4 * self.CW
        c = b + 4 * M
        d = c + 8 * self.MW * M
        return a, b, c, d, d + 4 * ((P + 3) // 4)


def bound(depth):
    s = Shape(depth)
    return s.offsets(s.NT, s.n ** 3)[4]


def bricks_of(solid):
    """[cx, cy, cz] brick bytes of a dense [x, y, z] occupancy: bit (z&1) 4 + (y&1) 2 + (x&1)"""
    v = (np.asarray(solid) != 0).astype(np.uint8)
    out = np.zeros(tuple(s // 2 for s in v.shape), np.uint8)
    for x in range(2):
        for y in range(2):
            for z in range(2):
                out |= v[x::2, y::2, z::2] << (z * 4 + y * 2 + x)
    return out


def dense_of(bricks):
    n = bricks.shape[0]
    out = np.zeros((2 * n,) * 3, np.uint8)
    for x in range(2):
        for y in range(2):
            for z in range(2):
                out[x::2, y::2, z::2] = (bricks >> (z * 4 + y * 2 + x)) & 1
    return out


def tiles_of(bricks, s):
    """(NT, K): tile t = (tx T + ty) T + tz, local index q = (i E + j) E + k"""
    T, E = s.T, s.E
    return bricks.reshape(T, E, T, E, T, E).transpose(0, 2, 4, 1, 3, 5).reshape(s.NT, s.K)


def bricks_from_tiles(tiles, s):
    T, E = s.T, s.E
    return tiles.reshape(T, T, T, E, E, E).transpose(0, 3, 1, 4, 2, 5).reshape(s.n, s.n, s.n)


def mask_words(bits, s):
    """(.., K) booleans -> (.., MW) uint32: bit q % 32 of word q / 32"""
    padded = np.zeros(bits.shape[:-1] + (32 * s.MW,), np.uint8)
    padded[..., :s.K] = bits
    return np.packbits(padded, axis=-1, bitorder="little").view("<u4")


def solid_of(bricks):
    """the solid voxels of an array of brick bytes, a slice at a time: no array eight times the bricks' size"""
    flat = np.ascontiguousarray(bricks).reshape(-1)
    return sum(int(np.bincount(flat[at:at + (1 << 24)], minlength=256) @ POPCOUNT) for at in range(0, flat.size, 1 << 24))


def pack(solid, depth):
    assert np.asarray(solid).shape == (1 << depth,) * 3
    return pack_bricks(bricks_of(solid), depth)


def pack_bricks(bricks, depth):
    """the stream of the [cx, cy, cz] brick bytes of bricks_of: what the large volumes are packed from, which need no dense
    array then"""
    s = Shape(depth)
    assert np.asarray(bricks).shape == (s.n,) * 3 and bricks.dtype == np.uint8
    tiles = tiles_of(bricks, s)
    some, full = tiles != 0, tiles == 0xFF
    cls = np.where(~some.any(1), 0, np.where(full.all(1), 1, 2)).astype(np.uint32)
    mixed = np.flatnonzero(cls == 2)
    partial = some[mixed] & ~full[mixed]
    M, P = len(mixed), int(partial.sum())
    length = s.offsets(M, P)[4]
    solid_count = solid_of(tiles)
    head = struct.pack("<6IQQ6I", MAGIC, VERSION, depth, s.NT, M, P, length, solid_count, int((cls == 1).sum()), 0, 0, 0, 0, 0)
    fields = np.zeros(16 * s.CW, np.uint32)
    fields[:s.NT] = cls
    a = (fields.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(1).astype("<u4")
    b = partial.sum(1).astype("<u4")
    c = np.concatenate([mask_words(some[mixed], s), mask_words(full[mixed], s)], axis=1).astype("<u4")
    d = tiles[mixed][partial]
    out = head + a.tobytes() + b.tobytes() + c.tobytes() + d.tobytes() + bytes(-P % 4)
    assert len(out) == length
    return out


def header_of(stream):
    """the 16 header words"""
    return list(struct.unpack("<16I", bytes(stream[:64])))


def header_rule(stream, depth=None, n_bytes=None):
    """the first header rule the stream breaks, or None; depth None: any depth in 2..10"""
    n_bytes = len(stream) if n_bytes is None else n_bytes
    if n_bytes < 64:
        return "header-short"
    h = header_of(stream)
    if h[0] != MAGIC or h[1] != VERSION:
        return "magic-version"
    if not 2 <= h[2] <= 10 or (depth is not None and h[2] != depth):
        return "depth"
    s = Shape(h[2])
    M, P, full = h[4], h[5], h[10]
    if h[3] != s.NT:
        return "tiles"
    if any(h[11:16]):
        return "reserved"
    length = h[6] | (h[7] << 32)
    if length != n_bytes:
        return "length-argument"
    if length != s.offsets(M, P)[4]:
        return "length-formula"
    if M > s.NT or P > s.K * M or full + M > s.NT:
        return "count-limits"
    return None


def unpack(stream, depth):
    """the dense [x, y, z] occupancy, or (rule, where): the first canonical rule the stream breaks, in the header's order, and
    "tile <t>" / "byte <offset>" of its least offender (None for the rules that have none)"""
    out = unpack_bricks(stream, depth)
    return out if isinstance(out, tuple) else dense_of(out)


def unpack_bricks(stream, depth):
    """unpack, with the [cx, cy, cz] brick bytes in the dense array's place"""
    stream = bytes(stream)
    rule = header_rule(stream, depth)
    if rule:
        return rule, None
    s = Shape(depth)
    h = header_of(stream)
    M, P, full_claimed = h[4], h[5], h[10]
    solid_claimed = h[8] | (h[9] << 32)
    a, b, c, d, _ = s.offsets(M, P)
    A = np.frombuffer(stream, "<u4", s.CW, a)
    B = np.frombuffer(stream, "<u4", M, b)
    Cw = np.frombuffer(stream, "<u4", 2 * s.MW * M, c).reshape(M, 2, s.MW)
    D = np.frombuffer(stream, np.uint8, 4 * ((P + 3) // 4), d)
    fields = ((A[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)
    bad = np.flatnonzero(np.concatenate([fields[:s.NT] == 3, fields[s.NT:] != 0]))
    broken = {}
    if len(bad):
        broken["class-map"] = "tile %d" % bad[0]
    cls = fields[:s.NT]
    mixed = np.flatnonzero(cls == 2)
    if len(mixed) != M:
        broken["mixed-count"] = None
    n_full = int((cls == 1).sum())
    if n_full != full_claimed:
        broken["full-count"] = None
    held = mixed[:M]                                          # the mask rules are evaluated for the ranks below M
    some_w, full_w = Cw[:len(held), 0], Cw[:len(held), 1]
    bits = lambda w: np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=-1, bitorder="little")      # (tiles, 32 MW)
    some, full = bits(some_w).astype(bool), bits(full_w).astype(bool)
    n_partial = (some & ~full).sum(1)

    def first(flags, name):
        at = np.flatnonzero(flags)
        if len(at):
            broken[name] = "tile %d" % held[at[0]]

    first((full & ~some).any(1), "full-in-some")
    first((some | full)[:, s.K:].any(1), "mask-range")
    first(~some.any(1), "some-empty")
    first(full.sum(1) == s.K, "full-whole")
    first(n_partial != B[:len(held)], "partial-count")
    if int(n_partial.sum()) != P:
        broken["partial-sum"] = None
    at = np.flatnonzero((D[:P] == 0) | (D[:P] == 0xFF))
    if len(at):
        broken["partial-byte"] = "byte %d" % (d + at[0])
    at = np.flatnonzero(D[P:] != 0)
    if len(at):
        broken["padding"] = "byte %d" % (d + P + at[0])
    counted = 8 * s.K * n_full + 8 * int(full.sum()) + solid_of(D[:P])
    if counted != solid_claimed:
        broken["solid-count"] = None
    for rule in DEVICE_RULES:
        if rule in broken:
            return rule, broken[rule]
    tiles = np.zeros((s.NT, s.K), np.uint8)
    tiles[cls == 1] = 0xFF
    mixed_tiles = np.where(full[:, :s.K], 0xFF, 0).astype(np.uint8)
    mixed_tiles[(some & ~full)[:, :s.K]] = D[:P]
    tiles[mixed] = mixed_tiles
    return bricks_from_tiles(tiles, s)


def set_words(stream, at, *values):
    out = bytearray(stream)
    out[at:at + 4 * len(values)] = struct.pack("<%dI" % len(values), *values)
    return bytes(out)


def corrupt(stream, rule, variant=0):
    """A stream that breaks `rule` of the valid `stream` and, where that forces more, only rules later in the order; None
    where this stream cannot break it (mask-range above depth 2, padding with P % 4 == 0, class-map variant 1 without unused
    fields, a rule that needs a tile of a class the stream lacks).  Returns (bytes, where) with where as unpack names it."""
    stream = bytes(stream)
    h = header_of(stream)
    s = Shape(h[2])
    M, P, n_full = h[4], h[5], h[10]
    a, b, c, d, length = s.offsets(M, P)
    fields = ((np.frombuffer(stream, "<u4", s.CW, a)[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)
    cls = fields[:s.NT]

    def with_class(t, value):
        word = struct.unpack_from("<I", stream, a + 4 * (t // 16))[0]
        word = (word & ~(3 << (2 * (t % 16)))) | (value << (2 * (t % 16)))
        return set_words(stream, a + 4 * (t // 16), word)

    def tile_of_class(value):
        at = np.flatnonzero(cls == value)
        return int(at[len(at) // 2]) if len(at) else None

    def masks(r):
        w = struct.unpack_from("<%dI" % (2 * s.MW), stream, c + 8 * s.MW * r)
        return list(w[:s.MW]), list(w[s.MW:])

    mixed = np.flatnonzero(cls == 2)
    r = M // 2                                                # the mixed tile the mask corruptions take
    if rule == "header-short":
        return stream[:60], None
    if rule == "magic-version":
        return (set_words(stream, 0, MAGIC ^ 0x100) if variant == 0 else set_words(stream, 4, 2)), None
    if rule == "depth":
        return set_words(stream, 8, 11 if variant == 0 else h[2] + 1 if h[2] < 10 else h[2] - 1), None
    if rule == "tiles":
        return set_words(stream, 12, s.NT + 1), None
    if rule == "reserved":
        return set_words(stream, 44 + 4 * (variant % 5), 1), None
    if rule == "length-argument":
        return (stream + bytes(4) if variant == 0 else set_words(stream, 28, 1)), None
    if rule == "length-formula":
        return set_words(stream, 20, P + 4), None
    if rule == "count-limits":
        return set_words(stream, 40, s.NT - M + 1), None
    if rule == "class-map":
        if variant == 1:
            return (with_class(s.NT, 1), "tile %d" % s.NT) if s.NT % 16 else None
        t = tile_of_class(0)
        return None if t is None else (with_class(t, 3), "tile %d" % t)
    if rule == "mixed-count":
        t = tile_of_class(0)
        return None if t is None else (with_class(t, 2), None)
    if rule == "full-count":
        t = tile_of_class(0)
        return None if t is None else (with_class(t, 1), None)
    if rule == "solid-count":
        return set_words(stream, 32, (h[8] + 1) & 0xFFFFFFFF), None
    if rule == "partial-sum":
        if P == 0 or P + 1 > s.K * M:
            return None
        return set_words(stream, 20, P + 1 if P % 4 else P - 1), None
    if rule == "partial-byte":
        if P == 0:
            return None
        at = d + (P // 2 if variant == 0 else P - 1)
        return stream[:at] + bytes([0 if variant == 0 else 0xFF]) + stream[at + 1:], "byte %d" % at
    if rule == "padding":
        if P % 4 == 0:
            return None
        return stream[:length - 1] + b"\x01", "byte %d" % (length - 1)
    if M == 0:
        return None
    where = "tile %d" % mixed[r]
    some, full = masks(r)
    if rule == "partial-count":
        count = struct.unpack_from("<I", stream, b + 4 * r)[0]
        return set_words(stream, b + 4 * r, count + 1), where
    if rule == "full-in-some":
        for q in range(s.K):                                  # an empty brick claimed full; failing that, a partial one
            if not (some[q // 32] >> (q % 32)) & 1:
                break
        else:
            q = next(q for q in range(s.K) if not (full[q // 32] >> (q % 32)) & 1)
        some[q // 32] &= ~(1 << (q % 32))
        full[q // 32] |= 1 << (q % 32)
    elif rule == "mask-range":
        if s.K >= 32:
            return None
        some[0] |= 1 << (s.K + variant)
    elif rule == "some-empty":
        some, full = [0] * s.MW, [0] * s.MW
    elif rule == "full-whole":
        whole = [0xFFFFFFFF] * s.MW if s.K >= 32 else [(1 << s.K) - 1]
        some, full = whole, list(whole)
    else:
        raise ValueError(rule)
    return set_words(stream, c + 8 * s.MW * r, *some, *full), where


def boundaries(stream):
    """the byte offsets at which the sections of a valid stream start and end: 64, B, C, D, the length"""
    h = header_of(stream)
    return sorted(set(Shape(h[2]).offsets(h[4], h[5])))


# ---- the fields the tests share ----------------------------------------------------------------------------------

def whole_brick_field(depth, rng, density=0.5):
    """every brick empty or full: mixed tiles (M > 0) without a partial brick (P = 0)"""
    n = 1 << (depth - 1)
    on = rng.random((n, n, n)) < density
    on.flat[0], on.flat[1:4] = True, False                    # both kinds, and three empty bricks, whatever the draw
    return np.repeat(np.repeat(np.repeat(on, 2, 0), 2, 1), 2, 2).astype(np.uint8)


def fields(depth):
    """(name, dense [x, y, z] uint8) for every field of the issue's list at `depth`"""
    S = 1 << depth
    rng = np.random.default_rng(900 + depth)
    out = [("random %.2f" % p, (rng.random((S, S, S)) < p).astype(np.uint8)) for p in (0.02, 0.5, 0.98)]
    out += [("empty", np.zeros((S, S, S), np.uint8)), ("full", np.ones((S, S, S), np.uint8))]
    box = np.zeros((S, S, S), np.uint8)
    edge = min(16, S // 2)                                    # a tile's edge in voxels from 32^3 up: whole tiles and half of one
    box[:edge, :edge, :edge] = 1
    box[edge:edge + edge // 2, :edge, :edge] = 1
    out.append(("tile-aligned box", box))
    x, y, z = np.ogrid[:S, :S, :S]
    c, r = S / 2 - 0.5, 0.4 * S
    out.append(("sphere", ((x - c) ** 2 + (y - c + 1) ** 2 + (z - c) ** 2 <= r * r).astype(np.uint8)))
    whole = whole_brick_field(depth, rng)
    out.append(("whole bricks", whole))
    for k in (1, 2, 3):                                       # P % 4 = k: single voxels in k empty bricks
        f = whole.copy()
        empty = np.argwhere(bricks_of(f) == 0)
        assert len(empty) >= k
        for cx, cy, cz in empty[:: max(1, len(empty) // k)][:k]:
            f[2 * cx + 1, 2 * cy, 2 * cz + 1] = 1
        out.append(("P %% 4 = %d" % k, f))
    return out


def corruptions(stream):
    """[(rule, variant, bytes, where)] for every rule corrupt() can break in `stream`"""
    out = []
    for rule in RULES:
        for variant in (0, 1):
            if variant == 1 and rule not in ("magic-version", "depth", "length-argument", "class-map", "partial-byte"):
                continue
            made = corrupt(stream, rule, variant)
            if made is not None:
                out.append((rule, variant, made[0], made[1]))
    return out
