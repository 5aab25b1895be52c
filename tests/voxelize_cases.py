"""The cases of tests/test_gpu_volume_voxelize_large.py: meshes under which the two kernels of vrc_volume_xor_mesh
(csrc/vrc_voxelize.hip) reach what the small tests do not -- the column scan at 2, 16, 32 and 64 lanes a brick column and at
two words a lane (depths 4, 7, 8, 9, 10), and the mark loop in a second and later step of its stride (split = 1, 1 < split <
useful, and the cap of 1024 workgroups a triangle at depth 10).  Beside the meshes and their expected flips: the launch
geometry of the two kernels restated in Python from the code as it stands, each with the line it was read off, and the scan
and the mark loop emulated in numpy with switches for wrong kernels, so that the host test
(tests/test_volume_voxelize_cases_host.py) can hold every case to the regime it is meant for and show that a wrong kernel
would change its result.  Expected results are sparse (voxelize_model.reduced rows (x, y, k): column (x, y) flipped on
[0, k)); they follow from how a case is made -- a one-column sheet at height k flips [0, k), a pair of tilted sheets flips
the slab between them -- and the host test holds them equal to the model.  numpy and Python integers only.

The largest integers the cases reach are the depth-10 slab's: |N| + D comes to 2^52.1 there (the host test computes it in
Python integers and prints it), against the bound of 2^57 in the kernel's header, which a triangle reaches only with
|n.z| near 2^37 AND its plane 2^17 units from the column's voxel centres -- a sliver no slab over the volume is."""
import functools

import numpy as np

import voxelize_model as M

U = M.UNIT
GROUP = 256                          # vrc_voxelize.hip:158, 165, 167: dim3(256) of every launch
WAVE = 64


# ---- the launch geometry ----------------------------------------------------------------------------------------------

def n_words(depth):
    """vrc_voxelize.hip:150: 32-bit words of the mark field (one byte per brick)"""
    return (1 << (3 * (depth - 1))) // 4


def scan_geometry(depth):
    """vrc_voxelize.hip:163-168: (lanes per brick column, words per lane PER) of k_scan_columns; depth >= 3"""
    column_words = (1 << depth) >> 3
    return (column_words, 1) if column_words <= 64 else (64, 2)


def scan_groups(depth):
    """vrc_voxelize.hip:165, 167: workgroups of the scan"""
    per = scan_geometry(depth)[1]
    return (n_words(depth) // per + GROUP - 1) // GROUP


def useful(depth):
    """vrc_voxelize.hip:155: the workgroups that cover the largest bounding box, S^2 columns, once"""
    S = 1 << depth
    return (S * S + GROUP - 1) // GROUP


def split_rule(n, units):
    """vrc_voxelize.hip:154-157 and vrc_volume.hip: split_for, the one rule of both: 4096 workgroups in all, at most 1024 an
    item, at most those that cover `units` units of work once"""
    return max(1, min((4096 + n - 1) // n, 1024, (units + GROUP - 1) // GROUP))


def split(depth, n):
    """vrc_voxelize.hip:154-157: gridDim.y of k_mark_triangles for a list of n triangles"""
    return split_rule(n, (1 << depth) ** 2)


def lanes_per_triangle(depth, n):
    return split(depth, n) * GROUP


def stride_steps(items, lanes):
    """vrc_voxelize.hip:71: for (it = lane; it < items; it += lanes): the steps of the lane that takes the most"""
    return -(-items // lanes)


def visits(items, groups, loop="stride"):
    """how often the loop of vrc_voxelize.hip:71 takes each of `items` items on `groups` workgroups of 256: ones as it stands;
    loop="once": no increment, the items beyond the first pass are dropped; loop="group": it += blockDim.x alone, so the
    lane of workgroup g also takes what the workgroups above g take"""
    it = np.arange(items, dtype=np.int64)
    if loop == "stride":
        return np.ones(items, np.int64)
    if loop == "once":
        return (it < groups * GROUP).astype(np.int64)
    assert loop == "group"
    return np.minimum(it // GROUP + 1, groups)                # the workgroups g <= it / 256 reach item it


def triangle_items(S, t):
    """items of a triangle's loop: the columns of its clipped bounding box (vrc_voxelize.hip:67-68), 0 where it returns early"""
    cols = M.triangle_columns(S, t)
    return 0 if cols is None else cols[2].size


def mark_rows(depth, tris, loop="stride", clamp=True):
    """the marks k_mark_triangles toggles, as unreduced rows (x, y, k) (the bit is voxel k - 1 of the column): item `it` of a
    triangle is column (lo.x + it / ncy, lo.y + it % ncy) (vrc_voxelize.hip:72), covered[x, y] in row-major order; an item
    the loop takes an even number of times toggles nothing.  clamp=False: k is not clamped to S (vrc_voxelize.hip:82)"""
    S = 1 << depth
    tris = np.asarray(tris).reshape(-1, 9)
    groups = split(depth, len(tris))
    rows = []
    for t in tris:
        cols = M.triangle_columns(S, t, clamp)
        if cols is None:
            continue
        x0, y0, covered, k = cols
        taken = (visits(covered.size, groups, loop) % 2 == 1).reshape(covered.shape)
        ix, iy = np.nonzero(covered & taken & (k > 0))
        rows.append(np.stack([ix + x0, iy + y0, k[ix, iy]], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)


# ---- the mark field and the scan --------------------------------------------------------------------------------------

def mark_words(depth, rows):
    """(words, bits) of the mark field after the rows (x, y, k) were toggled, the non-zero words in ascending order
    (vrc_voxelize.hip:83-85).  A k above S, which only a wrong kernel gives, lands where the linear brick index puts it, and
    is left out beyond the field"""
    S = 1 << depth
    n = S >> 1
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2] - 1
    brick = ((x >> 1) * n + (y >> 1)) * n + (z >> 1)
    word = brick >> 2
    bit = (((z & 1) * 4 + (y & 1) * 2 + (x & 1)) + 8 * (brick & 3)).astype(np.uint32)
    inside = word < n_words(depth)
    words, inverse = np.unique(word[inside], return_inverse=True)
    bits = np.zeros(len(words), np.uint32)
    np.bitwise_xor.at(bits, inverse, np.uint32(1) << bit[inside])
    return words[bits != 0], bits[bits != 0]


def flip_words(depth, flips):
    """(words, bits) of the occupancy words reduced flips change, ascending: the records vrc_delta_diff gives for the
    volume before and after (tests/delta_model.py: word = key >> 5)"""
    S = 1 << depth
    n = S >> 1
    runs = M.runs_of_flips(flips)
    x, y, z0, z1 = runs.T
    w0, w1 = z0 >> 3, (z1 - 1) >> 3
    count = w1 - w0 + 1
    which = np.repeat(np.arange(len(runs)), count)
    kz = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count) + w0[which]
    lo = np.maximum(z0[which] - 8 * kz, 0)
    hi = np.minimum(z1[which] - 8 * kz, 8)                                    # layers [lo, hi) of the word
    layers = ((np.uint64(1) << (4 * hi).astype(np.uint64)) - np.uint64(1)) ^ ((np.uint64(1) << (4 * lo).astype(np.uint64)) - np.uint64(1))
    bits = ((layers & np.uint64(0x11111111)) << ((y[which] & 1) * 2 + (x[which] & 1)).astype(np.uint64)).astype(np.uint32)
    word = ((x[which] >> 1) * n + (y[which] >> 1)) * (S >> 3) + kz
    words, inverse = np.unique(word, return_inverse=True)
    out = np.zeros(len(words), np.uint32)
    np.bitwise_xor.at(out, inverse, bits)
    return words[out != 0], out[out != 0]


def popcount(bits):
    b = np.asarray(bits, np.uint32).astype(np.uint64)
    b = b - ((b >> np.uint64(1)) & np.uint64(0x55555555))
    b = (b & np.uint64(0x33333333)) + ((b >> np.uint64(2)) & np.uint64(0x33333333))
    b = (b + (b >> np.uint64(4))) & np.uint64(0x0f0f0f0f)
    return int(((b * np.uint64(0x01010101)) >> np.uint64(24) & np.uint64(0xff)).sum())


def words_differing(a, b):
    """voxels at which two sparse word lists (words, bits) differ"""
    words = np.union1d(a[0], b[0])
    x = np.zeros(len(words), np.uint32)
    x[np.searchsorted(words, a[0])] ^= a[1]
    x[np.searchsorted(words, b[0])] ^= b[1]
    return popcount(x)


def suffix_xor(w):
    """vrc_voxelize.hip:90-94: nibble j of the result = XOR of the nibbles j.. of w"""
    w = w ^ (w >> np.uint32(4))
    w = w ^ (w >> np.uint32(8))
    return w ^ (w >> np.uint32(16))


SCAN_SWITCHES = ("no_guard", "stop_early", "wrong_pos", "ascending", "no_handoff", "own_one_word")


def scan(depth, marks, wrong=None):
    """k_scan_columns<PER> (vrc_voxelize.hip:98-126) on a sparse mark field (words, bits): the (words, bits) it XORs into the
    occupancy.  Waves of 64 lanes, lane l of wave v owns the words [(64 v + l) PER, +PER); __shfl_down(x, d) is a shift
    within the wave, and a lane whose source lies beyond the wave reads its own value.  Only the waves that hold a mark are
    emulated: the others leave at the ballot (line 111).  wrong: one of SCAN_SWITCHES --
      no_guard      line 117 without `pos + d < lanes`
      stop_early    line 115 with `d < lanes / 2`
      wrong_pos     line 113 with `threadIdx.x & (lanes * 2 - 1)`
      ascending     line 120 walks the lane's words upwards
      no_handoff    line 122 dropped: the carry is not handed from a word to the one below it in the lane
      own_one_word  line 108 with `=` for `^=`: own is the last word's alone"""
    assert wrong is None or wrong in SCAN_SWITCHES
    lanes, per = scan_geometry(depth)
    words, bits = marks
    thread = words // per
    waves = np.unique(thread // WAVE)
    m = np.zeros((len(waves), WAVE, per), np.uint32)
    m[np.searchsorted(waves, thread // WAVE), thread % WAVE, words % per] = bits
    f = suffix_xor(m)
    own = f[:, :, per - 1] & np.uint32(0xf) if wrong == "own_one_word" else np.bitwise_xor.reduce(f & np.uint32(0xf), axis=2)
    tid = (waves[:, None] % (GROUP // WAVE)) * WAVE + np.arange(WAVE)[None, :]             # threadIdx.x
    pos = tid & ((lanes * 2 - 1) if wrong == "wrong_pos" else (lanes - 1))
    incl = own.copy()
    d = 1
    while d < (lanes // 2 if wrong == "stop_early" else lanes):
        other = incl.copy()                                                 # out of range: the lane's own value
        other[:, :WAVE - d] = incl[:, d:]
        take = np.ones_like(pos, bool) if wrong == "no_guard" else pos + d < lanes
        incl = np.where(take, incl ^ other, incl)
        d <<= 1
    carry = incl ^ own
    flips = np.zeros_like(m)
    for j in (range(per) if wrong == "ascending" else range(per - 1, -1, -1)):
        flips[:, :, j] = f[:, :, j] ^ (carry * np.uint32(0x11111111))
        if wrong != "no_handoff":
            carry = flips[:, :, j] & np.uint32(0xf)
    v, l, j = np.nonzero(flips)
    out = (waves[v] * WAVE + l) * per + j
    order = np.argsort(out)
    return out[order], flips[v, l, j][order]


def voxels_changed(depth, tris, wrong):
    """how many voxels of the result of xorMesh(tris) at `depth` a wrong kernel changes: a scan switch, or "once" / "group"
    (the mark loop) or "no_clamp" (k not clamped to S)"""
    right = mark_rows(depth, tris)
    S = 1 << depth
    if wrong in SCAN_SWITCHES:
        marks = mark_words(depth, M.reduced(S, right))
        return words_differing(scan(depth, marks, wrong), scan(depth, marks))
    rows = mark_rows(depth, tris, clamp=False) if wrong == "no_clamp" else mark_rows(depth, tris, loop=wrong)
    if wrong != "no_clamp":
        return M.count_of_flips(M.reduced(S, np.concatenate([right, rows])))          # the scan is linear in the marks
    beyond = rows[:, 2] > S                                                   # right and rows are in the same order
    return popcount(scan(depth, mark_words(depth, np.concatenate([right[beyond], rows[beyond]])))[1])


# ---- meshes -----------------------------------------------------------------------------------------------------------

def sheet(x0, y0, x1, y1, h):
    """an open horizontal rectangle [x0, x1] x [y0, y1] (voxels) at height h (units): two triangles"""
    a, b, c, d = (x0 * U, y0 * U, h), (x1 * U, y0 * U, h), (x1 * U, y1 * U, h), (x0 * U, y1 * U, h)
    return np.array([a + b + c, a + c + d], np.int32)


def column_sheets(cols):
    """one-column sheets for rows (x, y, k): column (x, y) is flipped on [0, min(k, S)); the sheet lies k voxels up, above the
    volume where k > S"""
    return np.concatenate([sheet(x, y, x + 1, y + 1, k * U) for x, y, k in np.asarray(cols).tolist()])


def tilted(lo, hi, h0, sx, sy):
    """a rectangle [lo, hi]^2 (voxels, in x and y) in the plane z = h0 + sx x + sy y (h0 in units, sx and sy even, units a
    voxel): two triangles"""
    assert sx % 2 == 0 and sy % 2 == 0
    z = lambda x, y: h0 + sx * x + sy * y
    a, b, c, d = (lo * U, lo * U, z(lo, lo)), (hi * U, lo * U, z(hi, lo)), (hi * U, hi * U, z(hi, hi)), (lo * U, hi * U, z(lo, hi))
    return np.array([a + b + c, a + c + d], np.int64).astype(np.int32)


def tilted_k(S, h0, sx, sy):
    """k per column [x, y] under tilted(...) where that covers the whole volume: the plane at the column's centre is
    h0 + sx x + sy y + (sx + sy) / 2, an integer, and k = clamp(ceil((that - 32) / 64), 0, S)"""
    x, y = np.arange(S, dtype=np.int64)[:, None], np.arange(S, dtype=np.int64)[None, :]
    return np.clip((h0 + sx * x + sy * y + (sx + sy) // 2 + 31) // U, 0, S)


def slab(S, lo, hi, h0, sx, sy, rise):
    """a tilted sheet over the whole volume and its copy `rise` voxels higher: (4 triangles, the rows (x, y, k) of both)"""
    tris = np.concatenate([tilted(lo, hi, h0, sx, sy), tilted(lo, hi, h0 + rise * U, sx, sy)])
    x, y = [g.reshape(-1) for g in np.meshgrid(np.arange(S), np.arange(S), indexing="ij")]
    rows = np.concatenate([np.stack([x, y, tilted_k(S, h, sx, sy).reshape(-1)], axis=1) for h in (h0, h0 + rise * U)])
    return tris, rows


def tetrahedra(S, count, rng):
    """`count` closed tetrahedra, each inside one voxel's cube, some at the volume's faces: 4 triangles each"""
    corner = rng.integers(-1, S, (count, 1, 3)) * U
    v = corner + rng.integers(0, U + 1, (count, 4, 3))
    faces = np.array([(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)])
    return v[:, faces, :].reshape(-1, 9).astype(np.int32)


class Case:
    """depth, tris, flips (reduced rows) and what a case wants to say besides"""

    def __init__(self, depth, tris, flips, **more):
        self.depth, self.S, self.tris, self.flips = depth, 1 << depth, np.ascontiguousarray(tris, np.int32), flips
        self.__dict__.update(more)


# ---- the scan cases ---------------------------------------------------------------------------------------------------

SCAN_DEPTHS = (4, 7, 8, 9, 10)


def brick_columns(depth, pairs):
    """`pairs` pairs (b, b + 1) of brick columns, b even, no column twice: neighbours in a wave wherever a wave holds more
    than one column (depths 4, 7, 8).  The first pair is columns 0 and 1, the last n^2 - 2 and n^2 - 1, the others 2042
    columns apart (1021 at depth 4), so that they fall into different waves and workgroups and, at 16 lanes a column, into
    the lower and the upper half of a wave in turn"""
    half = (1 << (2 * (depth - 1))) // 2
    assert pairs <= half
    base = [2 * (p * 1021 % half) for p in range(pairs - 1)] + [2 * half - 2]
    assert len(set(base)) == pairs
    return base


def voxel_column(depth, b, xb, yb):
    n = 1 << (depth - 1)
    return 2 * (b // n) + xb, 2 * (b % n) + yb


@functools.lru_cache(maxsize=None)
def scan_case(depth):
    """Every scan case of one depth in one list of sheets, each part in brick columns of its own.  Shared: do not write to it.
      borders     for every word border j of a column, k = 8 j and 8 j + 1, then a sheet above the volume and k = S: every
                  lane hands a carry down over every distance.  The first is k = 1 in brick column 0 (word 0), the last k = S
                  in the last brick column (word n_words - 1)
      crossings   k1 < k2 in one column, in different lanes; at depth 10 also in the two words of one lane
      neighbours  of a pair (A, A + 1) one column marked at its lowest and at its highest voxel and the other not, both ways
                  round, and once more with the top mark alone
      cancelled   two sheets, each twice, in a brick column of their own: the marks cancel
      layer       300 sheets at random columns of a 16 x 16 block and random heights, every tenth a repeat of an earlier one
                  (it cancels), every seventh in an earlier one's brick and word
    .parts names the rows of each; .flips is the reduction of all rows"""
    S = 1 << depth
    W = S >> 3
    rng = np.random.default_rng(1000 + depth)
    ks = [k for j in range(W) for k in (8 * j, 8 * j + 1) if k] + [S - 1, S + 3, S]       # an even number: k = S is the odd one of its pair
    crossings = [(3, S - 2), (8 + 2, S - 9), (S // 2 - 3, S // 2 + 6)]
    if depth == 10:
        crossings += [(16 * L + 5, 16 * L + 8 + 3) for L in (0, 37, 63)]
    pairs = brick_columns(depth, (len(ks) + 1) // 2 + len(crossings) + 3 + 1 + 1)
    cols = pairs[:(len(ks) + 1) // 2 - 1] + pairs[-1:]                      # borders: the first pairs and the last
    rest = pairs[(len(ks) + 1) // 2 - 1:-1]
    parts = {"borders": [], "crossings": [], "neighbours": [], "cancelled": [], "layer": []}
    for i, k in enumerate(ks):
        b = cols[i // 2] + (i & 1)
        last = i == len(ks) - 1                                             # k = S in column (S - 1, S - 1)
        parts["borders"].append(voxel_column(depth, b, 1 if last else (i >> 1) & 1, 1 if last else ((i >> 2) ^ i) & 1) + (k,))
    for i, (k1, k2) in enumerate(crossings):
        x, y = voxel_column(depth, rest[i] + (i & 1), i & 1, (i >> 1) & 1)
        parts["crossings"] += [(x, y, k1), (x, y, k2)]
    empty = []                                                              # brick columns that must stay empty
    for i, (marked, other, both) in enumerate(((1, 0, True), (0, 1, True), (1, 0, False))):
        b = rest[len(crossings) + i]
        x, y = voxel_column(depth, b + marked, 1, 0)
        parts["neighbours"] += ([(x, y, 1)] if both else []) + [(x, y, S)]
        empty.append(b + other)
    x, y = voxel_column(depth, rest[len(crossings) + 3] + 1, 0, 1)           # every sheet twice: the marks cancel, the words stay
    parts["cancelled"] = [(x, y, 5), (x, y, S - 2), (x, y, 5), (x, y, S - 2)]
    empty.append(rest[len(crossings) + 3] + 1)
    x0, y0 = voxel_column(depth, rest[len(crossings) + 4], 0, 0)
    side = min(16, S // 4)
    x0, y0 = min(x0, S - side), min(y0, S - side)
    layer = []
    for i in range(300):
        if i % 10 == 9:
            layer.append(layer[int(rng.integers(0, len(layer)))])
        elif i % 7 == 6:
            x, y, k = layer[int(rng.integers(0, len(layer)))]
            layer.append((x ^ 1, y, ((k - 1) | 7) + 1 - int(rng.integers(0, 8))))
        else:
            layer.append((x0 + int(rng.integers(0, side)), y0 + int(rng.integers(0, side)), int(rng.integers(1, S + 1))))
    parts["layer"] = layer
    parts = {name: np.array(rows, np.int64) for name, rows in parts.items()}
    rows = np.concatenate([parts[name] for name in ("borders", "crossings", "neighbours", "cancelled", "layer")])
    flips = M.reduced(S, np.minimum(rows, [S, S, S]))
    return Case(depth, column_sheets(rows), flips, parts=parts, empty_bricks=empty)


def before_boxes(depth):
    """what the non-empty volume holds before the call, as fill_boxes boxes that do not overlap: a slab through every column
    (z in [S/4, S/4 + S/8)), the lowest layer of a quarter of the volume, a block in the far corner and, in the layer's block,
    a few whole columns"""
    S = 1 << depth
    return np.array([[0, 0, S // 4, S, S, S // 4 + S // 8], [0, 0, 0, S // 2, S // 2, 1], [S - 5, S - 7, S - 3, S, S, S],
                     [2, 2, S // 2, 3, S - 9, S // 2 + min(9, S // 4)]], np.uint32)


def solid_in_boxes(boxes, runs):
    """voxels of the runs (x, y, z0, z1) that lie in the (disjoint) boxes"""
    x, y, z0, z1 = np.asarray(runs, np.int64).T
    total = 0
    for bx0, by0, bz0, bx1, by1, bz1 in np.asarray(boxes, np.int64).tolist():
        inside = (x >= bx0) & (x < bx1) & (y >= by0) & (y < by1)
        total += int(np.maximum(np.minimum(z1, bz1) - np.maximum(z0, bz0), 0)[inside].sum())
    return total


def boxes_volume(boxes):
    b = np.asarray(boxes, np.int64)
    return int(np.prod(b[:, 3:] - b[:, :3], axis=1).sum())


def dense_boxes(S, boxes):
    vol = np.zeros((S, S, S), np.uint8)
    for x0, y0, z0, x1, y1, z1 in np.asarray(boxes, np.int64).tolist():
        vol[x0:x1, y0:y1, z0:z1] = 1
    return vol


# ---- the stride cases -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def stride_case(depth, n=None):
    """Slab pairs over the whole volume among small closed tetrahedra, n triangles in all.  Shared: do not write to it.
      depth 5            4112 triangles, split = 1: a slab pair first, in the middle and last; 1024 columns on 256 lanes
      depth 7, n = 128   split = 32: 16384 columns on 8192 lanes, two full steps
      depth 7, n = 150   split = 28: 7168 lanes, three steps, the last of 2048 items
      depth 9, n = 8     split = 512: 262144 columns on 131072 lanes, two steps
      depth 10, n = 4    split = 1024, the cap: 2^20 columns on 262144 lanes, four steps; the rectangle's corners lie at
                         +-2^17 units in x and y
    Every slab rises above the volume's top in a corner, where k is clamped to S.  .slab_rows are the rows of the slabs by
    their construction, .flips the expectation: the reduction of the slabs' rows and the model's for the tetrahedra"""
    S = 1 << depth
    rng = np.random.default_rng(2000 + depth)
    if depth == 10:
        tris, rows = slab(S, -2048, 2048, 600 * U, 16, 16, 3)
        return Case(depth, tris, M.reduced(S, rows), slab_rows=rows, slabs=tris, n=4)
    # the planes: from S/3 up to above the top at the far corner, each pair with slopes of its own
    planes = [(S * U // 3, 2 * (12 + i), 2 * (14 - i), 2 + i) for i in range(3)]
    made = [slab(S, -1, S + 1, *p) for p in planes]
    if depth == 5:
        small = tetrahedra(S, 1025, rng)
        tris = np.concatenate([made[0][0], small[:2048], made[1][0], small[2048:], made[2][0]])
        used = made
    elif depth == 9:
        small = np.zeros((0, 9), np.int32)
        tris = np.concatenate([made[0][0], made[1][0]])
        used = made[:2]
    else:
        small = tetrahedra(S, (n - 8) // 4, rng)                              # and a one-column sheet where that leaves two
        extra = sheet(5, 9, 6, 10, 40 * U) if (n - 8) % 4 else np.zeros((0, 9), np.int32)
        tris = np.concatenate([small[:40], made[0][0], small[40:], extra, made[1][0]])
        small = np.concatenate([small, extra])
        used = made[:2]
    assert n is None or len(tris) == n
    rows = np.concatenate([r for _, r in used])
    flips = M.reduced(S, np.concatenate([rows, M.column_flips(S, small)]))
    return Case(depth, tris, flips, slab_rows=rows, slabs=np.concatenate([t for t, _ in used]), n=len(tris))


STRIDE_CASES = ((5, None), (7, 128), (7, 150), (9, None), (10, None))


# ---- end to end -------------------------------------------------------------------------------------------------------

STAMP = dict(depth=8, subdivisions=3, radius=75.3, centre=(131.4, 140.7, 97.2))      # about 150 voxels across: a 256^3 clipboard


def stamp_flips(verts, faces):
    """the flips of the stamped icosphere in the 256^3 world, by the model"""
    return M.column_flips(256, M.soup(M.quantise(verts, STAMP["radius"], STAMP["centre"]), faces))
