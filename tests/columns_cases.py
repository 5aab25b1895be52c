"""The cases of tests/test_gpu_volume_columns_planes.py: columns whose counters reach the high bit-planes of
csrc/vrc_columns.hip.  The two walks keep first, last, count and runs of the 16 (4) columns of a bundle as bit-planes over the
column positions of a level, and the select keeps P - lo and P - hi as two's-complement planes; plane b of a number holds a one
only once the number reaches 2^b, so a coordinate's or a run count's plane b needs S = 2^(b + 1) and count's plane 10 needs
S = 1024.  Columns are sparse: a scene is a few hundred programmed columns in an otherwise empty volume, built from one box a
run, and its expected records and selections follow from the run lists -- nothing dense exists above 128^3.
  a. column programs, the catalogue as a function of S, the placement over bundles, the sparse model;
  b. the launch geometry, the word layout and the walks of k_columns_profile / k_columns_select restated from the code as it
     stands, each with the line it was read off, emulated word by word and vectorised over bundles, with switches for
     wrong kernels;
  c. the scenes of tests/test_gpu_volume_columns.py at 128^3, 256^3 and 1024^3 as words, for the same emulation.
tests/test_volume_columns_cases_host.py holds all of it to its regime without a GPU.  numpy and Python integers only."""
import functools

import numpy as np

import cells_model
import columns_model as model

NONE = model.NONE
SOLID, EMPTY, BOTH = model.SOLID, model.EMPTY, model.BOTH
M32 = 0xFFFFFFFF
EMPTY_RECORD = (NONE, NONE, 0, 0)

# ---- the geometry, restated ----------------------------------------------------------------------------------------------

COUNT_PLANES, COORD_PLANES, SIGNED_PLANES, WALK_GROUP = 11, 10, 12, 64         # vrc_columns.hip:38-41
LEVELS = (2, 2, 8)                                                             # vrc_columns.hip:45
SHIFT = (1, 2, 4)                                                              # vrc_columns.hip:46
COLUMNS = (0x55555555, 0x33333333, 0xF)                                        # vrc_columns.hip:47
N_COLUMNS = (16, 16, 4)                                                        # vrc_columns.hip:48


def bundles(axis, u_lo, v_lo, u_hi, v_hi):
    """vrc_columns.hip:59-64: the grid (a0, na, b0, nb) of the bundles a rect touches"""
    vs = 1 if axis == 2 else 3
    return u_lo >> 1, ((u_hi - 1) >> 1) - (u_lo >> 1) + 1, v_lo >> vs, ((v_hi - 1) >> vs) - (v_lo >> vs) + 1


def column_of(axis, c, a, b):
    """vrc_columns.hip:67-74: (bit, u, v) of column c of bundle (a, b); c, a, b may be arrays"""
    hi, lo = c >> 1, c & 1
    if axis == 0:
        return 4 * hi + 2 * lo, 2 * a + lo, 8 * b + hi
    if axis == 1:
        return 4 * hi + lo, 2 * a + lo, 8 * b + hi
    return c, 2 * a + lo, 2 * b + hi


def bundle_of(axis, u, v):
    """column_of the other way round: (a, b, c) of the column (u, v)"""
    if axis == 2:
        return u >> 1, v >> 1, 2 * (v & 1) + (u & 1)
    return u >> 1, v >> 3, 2 * (v & 7) + (u & 1)


def face_bundles(axis, S):
    """(na, nb) of the whole face"""
    _, na, _, nb = bundles(axis, 0, 0, S, S)
    return na, nb


def lane_of(axis, S, a, b, rect=None):
    """vrc_columns.hip:130-132: it = (a - a0) nb + (b - b0); the workgroup is it // WALK_GROUP"""
    a0, _, b0, nb = bundles(axis, *(rect or (0, 0, S, S)))
    return (a - a0) * nb + (b - b0)


def groups_of(axis, rect):
    """vrc_columns.hip:260-261"""
    _, na, _, nb = bundles(axis, *rect)
    return (na * nb + WALK_GROUP - 1) // WALK_GROUP


def walk_of(axis, lg, a, b):
    """vrc_columns.hip:85-99: (idx, idx_step, shift, shift_step, mask, steps); a, b may be arrays"""
    n = 1 << lg
    if lg < 2:
        if axis == 0:
            return 0 * a, 1, 16 * a, 0, 0xFFFF, 2
        if axis == 1:
            return a, 0, 0 * a, 16, 0xFFFF, 2
        return a, 0, 16 * b, 0, 0xFFFF, 1
    nwz = n >> 2
    if axis == 0:
        return a * nwz + b, n * nwz, 0 * a, 0, M32, n
    if axis == 1:
        return a * n * nwz + b, nwz, 0 * a, 0, M32, n
    return (a * n + b) * nwz, 1, 0 * a, 0, M32, nwz


def word_of(S, x, y, z):
    """(index, bit) of a voxel: vrc_flood.hip:3-4, a word is 2 x 2 x 8 voxels, bit 4 k + 2 yb + xb with k = z & 7, the words
    of a brick row consecutive; 4^3: word cx, half cy (vrc_columns.hip:24-26)"""
    n = S >> 1
    if n < 4:
        return x >> 1, 16 * (y >> 1) + 4 * z + 2 * (y & 1) + (x & 1)
    return ((x >> 1) * n + (y >> 1)) * (n >> 2) + (z >> 3), 4 * (z & 7) + 2 * (y & 1) + (x & 1)


class Words:
    """the occupancy words of a volume, sparse: `fill` everywhere but at the sorted indices `at`, which hold `values`"""

    def __init__(self, S, at=(), values=(), fill=0):
        self.S, self.fill = S, np.uint32(fill)
        self.at, self.values = np.asarray(at, np.int64), np.asarray(values, np.uint32)

    def __getitem__(self, idx):
        if not len(self.at):
            return np.full(np.shape(idx), self.fill, np.uint32)
        pos = np.minimum(np.searchsorted(self.at, idx), len(self.at) - 1)
        return np.where(self.at[pos] == idx, self.values[pos], self.fill)

    @staticmethod
    def of_voxels(S, xyz, solid=True, fill=0):
        """`fill` with the voxels (n, 3) set (solid) or cleared"""
        xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
        idx, bit = word_of(S, xyz[:, 0], xyz[:, 1], xyz[:, 2])
        at, inverse = np.unique(idx, return_inverse=True)
        bits = np.zeros(len(at), np.uint32)
        np.bitwise_or.at(bits, inverse, (1 << bit).astype(np.uint32))
        return Words(S, at, bits if solid else np.uint32(fill) & ~bits, fill)

    @staticmethod
    def of_dense(vol):
        return Words.of_voxels(vol.shape[0], np.argwhere(np.asarray(vol) != 0))


def dense_of_words(words):
    """the dense [x, y, z] uint8 form of sparse words on an empty ground, S >= 8"""
    S, n = words.S, words.S >> 1
    assert n >= 4 and not words.fill
    V = np.zeros((S, S, S), np.uint8)
    at, bit = [g.reshape(-1) for g in np.meshgrid(np.arange(len(words.at)), np.arange(32), indexing="ij")]
    keep = ((words.values[at] >> bit.astype(np.uint32)) & 1).astype(bool)
    idx, bit = words.at[at[keep]], bit[keep]
    V[2 * (idx // ((n >> 2) * n)) + (bit & 1), 2 * (idx // (n >> 2) % n) + (bit >> 1 & 1), 8 * (idx % (n >> 2)) + (bit >> 2)] = 1
    return V


# ---- a. column programs ---------------------------------------------------------------------------------------------------

def normal(runs):
    """sorted, and runs that touch merged"""
    out = []
    for z0, z1 in sorted(runs):
        if out and z0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], z1))
        else:
            out.append((z0, z1))
    return tuple(out)


def powers(S):
    """B = {2^b : 2^b <= S / 2}"""
    return [1 << b for b in range((S // 2).bit_length())]


def around_powers(S, top=None):
    """{2^b - 1, 2^b, 2^b + 1} for the 2^b of B (or up to `top`), ascending"""
    return sorted({p + o for p in powers(2 * top if top else S) for o in (-1, 0, 1)})


def mixed(S):
    return [0x155 & (S - 1), 0x2AA & (S - 1)]


def catalogue(S):
    """[(name, runs)]: the programs of a column of S levels, pairwise different"""
    out = []
    for r in around_powers(S):                                  # combs: one-voxel runs, one-voxel gaps
        for start in (0, 1):
            if r >= 1 and start + 2 * r - 1 <= S:
                out.append(("comb %d from %d" % (r, start), [(start + 2 * i, start + 2 * i + 1) for i in range(r)]))
    r = S // 4 + 1                                              # two-voxel runs: count = 2 runs
    out.append(("comb of twos %d" % r, [(1 + 3 * i, 3 + 3 * i) for i in range(r)]))
    for c in sorted(set(around_powers(S) + mixed(S) + [S - 1, S])):             # counts: one run against either face and in the middle
        if 1 <= c <= S:
            for where, z0 in (("entry", 0), ("exit", S - c), ("middle", (S - c) // 2)):
                out.append(("count %d %s" % (c, where), [(z0, z0 + c)]))
    m1, m2 = mixed(S)
    pairs = [(m1, m2), (0, S - 1)]
    for p in powers(S):                                         # ends: two single voxels
        pairs += [(p - 1, p), (p, S - 1), (0, p + 1), (p - 1, m2), (m1, p + 1), (p + 1, S - 1), (p, m1)]
    for p, q in pairs:
        if 0 <= p < q <= S - 1:
            out.append(("ends %d %d" % (p, q), [(p, p + 1), (q, q + 1)]))
    e = 8 * (7 * S // 64)                                       # word seams along z: z = 8 w in the last quarter
    o = 7 * S // 8 + 1                                          # along x and y: the odd / even pair (o, o + 1) high up
    for at in sorted({e, o + 1}):
        out += [("seam ends at %d" % at, [(at - 3, at)]), ("seam starts at %d" % at, [(at, at + 3)]), ("seam straddles %d" % at, [(at - 2, at + 2)]),
                ("seam both sides of %d" % at, [(at - 2, at - 1), (at, at + 1)]), ("seam gap at %d" % at, [(at - 2, at), (at + 1, at + 2)])]
    seen, unique = set(), []
    for name, runs in out:
        runs = normal(runs)
        if runs not in seen:
            seen.add(runs)
            unique.append((name, runs))
    return unique


def record_tuple(runs, S, side):
    """the vrc_column of a column met along side 1 (up the axis) or 0, straight from its runs"""
    if not runs:
        return EMPTY_RECORD
    least, greatest = runs[0][0], runs[-1][1] - 1
    return (least if side else greatest), (greatest if side else least), sum(z1 - z0 for z0, z1 in runs), len(runs)


def merged(spans):
    return list(normal([s for s in spans if s[0] < s[1]]))


def selected_spans(runs, S, side, lo, hi, of):
    """the spans [z0, z1) of a column that vrc_columns_select takes: P of a voxel = solid voxels met before it.  In travel
    order the k-th solid voxel has P = k, and the empty voxels between two runs have the length of all runs before them"""
    travel = list(runs) if side else [(S - z1, S - z0) for z0, z1 in reversed(runs)]
    out, before, at = [], 0, 0
    for t0, t1 in travel:
        if of & EMPTY and lo <= before < hi:
            out.append((at, t0))
        if of & SOLID:
            k0, k1 = max(lo, before), min(hi, before + t1 - t0)
            out.append((t0 + k0 - before, t0 + k1 - before))
        before, at = before + t1 - t0, t1
    if of & EMPTY and lo <= before < hi:
        out.append((at, S))
    out = merged(out)
    return out if side else [(S - t1, S - t0) for t0, t1 in reversed(out)]


def box_of(axis, u, v, z0, z1):
    """x0 y0 z0 x1 y1 z1 of the levels [z0, z1) of column (u, v): (u, v) are the other two axes in x < y < z order"""
    lo, hi = [0, 0, 0], [0, 0, 0]
    o = [a for a in range(3) if a != axis]
    lo[axis], hi[axis] = z0, z1
    lo[o[0]], hi[o[0]], lo[o[1]], hi[o[1]] = u, u + 1, v, v + 1
    return lo + hi


def box_of_rect(axis, rect, z0, z1):
    """x0 y0 z0 x1 y1 z1 of the levels [z0, z1) of the columns of a rect (u_lo, v_lo, u_hi, v_hi)"""
    lo, hi = box_of(axis, rect[0], rect[1], z0, z1)[:3], box_of(axis, rect[2] - 1, rect[3] - 1, z0, z1)[3:]
    return lo + hi


class Scene:
    """depth, axis, columns [(u, v, runs)], and `placed` [(a, b, {c: index into columns})] -- the programmed bundles"""

    def __init__(self, depth, axis, columns, names=None):
        self.depth, self.S, self.axis = depth, 1 << depth, axis
        self.columns = [(u, v, normal(runs)) for u, v, runs in columns]
        self.names = names
        self.placed = {}
        for i, (u, v, _) in enumerate(self.columns):
            a, b, c = bundle_of(axis, u, v)
            assert c not in self.placed.setdefault((a, b), {})
            self.placed[a, b][c] = i

    def boxes(self):
        """one fillBoxes box per run"""
        return np.array([box_of(self.axis, u, v, z0, z1) for u, v, runs in self.columns for z0, z1 in runs], np.uint32).reshape(-1, 6)

    def dense(self):
        V = np.zeros((self.S,) * 3, np.uint8)
        for x0, y0, z0, x1, y1, z1 in self.boxes().tolist():
            V[x0:x1, y0:y1, z0:z1] = 1
        return V

    def words(self):
        xyz = [np.stack(np.broadcast_arrays(*[np.arange(b[i], b[i + 3]) for i in range(3)]), -1) for b in self.boxes().astype(np.int64)]
        return Words.of_voxels(self.S, np.concatenate(xyz)) if xyz else Words(self.S)

    def seen_along(self, axis):
        """the same voxels as the columns of another axis: a scene of its own, whose sparse model holds for that axis"""
        b = self.boxes().astype(np.int64)
        xyz = np.concatenate([np.stack(np.broadcast_arrays(*[np.arange(r[i], r[i + 3]) for i in range(3)]), -1) for r in b])
        o = [x for x in range(3) if x != axis]
        u, v, z = xyz[:, o[0]], xyz[:, o[1]], xyz[:, axis]
        order = np.lexsort((z, v, u))
        u, v, z = u[order], v[order], z[order]
        start = np.flatnonzero(np.concatenate([[True], (u[1:] != u[:-1]) | (v[1:] != v[:-1]) | (z[1:] != z[:-1] + 1)]))
        end = np.append(start[1:], len(z))
        columns = {}
        for i, j in zip(start.tolist(), end.tolist()):
            columns.setdefault((int(u[i]), int(v[i])), []).append((int(z[i]), int(z[j - 1]) + 1))
        return Scene(self.depth, axis, [(u, v, runs) for (u, v), runs in columns.items()])

    def solid(self):
        return sum(z1 - z0 for _, _, runs in self.columns for z0, z1 in runs)

    def profile(self, side, rect=None):
        """the sparse model: the records of a rect (the whole face), (U, V) COLUMN_DTYPE"""
        u_lo, v_lo, u_hi, v_hi = rect or (0, 0, self.S, self.S)
        out = np.empty((u_hi - u_lo, v_hi - v_lo), model.COLUMN_DTYPE)
        out[...] = EMPTY_RECORD
        for u, v, runs in self.columns:
            if u_lo <= u < u_hi and v_lo <= v < v_hi:
                out[u - u_lo, v - v_lo] = record_tuple(runs, self.S, side)
        return out

    def records(self, side):
        """[the record of every programmed column]"""
        return np.array([record_tuple(runs, self.S, side) for _, _, runs in self.columns], np.int64)

    def selection(self, side, lo, hi, of):
        """[the selected spans of every programmed column].  An empty column has P = 0 everywhere: with of = SOLID, or with
        lo >= 1, it selects nothing, and the selection stays inside the programmed columns"""
        assert of == SOLID or lo >= 1
        return [selected_spans(runs, self.S, side, lo, hi, of) for _, _, runs in self.columns]

    def selection_boxes(self, side, lo, hi, of):
        """(the spans as boxes (n, 6), the voxels of each)"""
        spans = self.selection(side, lo, hi, of)
        boxes = [box_of(self.axis, u, v, z0, z1) for (u, v, _), sp in zip(self.columns, spans) for z0, z1 in sp]
        return np.array(boxes, np.uint32).reshape(-1, 6), np.array([z1 - z0 for sp in spans for z0, z1 in sp], np.uint64)

    def selection_scene(self, side, lo, hi, of):
        """the selection as a scene of its own: its dense() and words() are the expected destination"""
        return Scene(self.depth, self.axis, [(u, v, sp) for (u, v, _), sp in zip(self.columns, self.selection(side, lo, hi, of))])


def bundle_lanes(axis, S, n_programs):
    """the whole-face lanes of the programmed bundles, in the order they are dealt: the last bundle of the face first, then
    down the face in equal odd strides of at least 3 -- empty bundles between any two, and many workgroups apart"""
    N = N_COLUMNS[axis]
    na, nb = face_bundles(axis, S)
    full = -(-(n_programs - N) // N)
    needed = full + N
    stride = max(3, ((na * nb - 1) // needed) | 1)
    return [na * nb - 1 - k * stride for k in range(needed)], full


@functools.lru_cache(maxsize=None)
def scene(depth, axis):
    """the catalogue of S dealt over bundles.  N = 16 (x, y) or 4 (z) columns a bundle:
      the N programs at equal distances through the catalogue go ONE to a bundle, at the positions c = 0 .. N - 1 in turn;
      the others are dealt round-robin over ceil(rest / N) bundles, a mix of combs, counts and ends in each; all of them are
      whole but the last one dealt to, and the first is the last bundle of the face (a, b both greatest)"""
    S = 1 << depth
    programs = catalogue(S)
    N = N_COLUMNS[axis]
    lanes, full = bundle_lanes(axis, S, len(programs))
    _, nb = face_bundles(axis, S)
    alone = [i * (len(programs) // N) for i in range(N)]
    rest = [i for i in range(len(programs)) if i not in alone]
    columns, names = [], []

    def place(lane, c, i):
        _, u, v = column_of(axis, c, lane // nb, lane % nb)
        columns.append((u, v, programs[i][1]))
        names.append(programs[i][0])

    sizes = [N] * (full - 1) + [len(rest) - N * (full - 1)]
    slots = [(k, c) for c in range(N) for k in range(full) if c < sizes[k]]     # round-robin: a bundle gets a mix of the catalogue
    for (k, c), i in zip(slots, rest):
        place(lanes[k], c, i)
    for c, i in enumerate(alone):
        place(lanes[full + c], c, i)
    return Scene(depth, axis, columns, names)


def bundle_rect(axis, S, a, b):
    """the rect of the columns of bundle (a, b)"""
    _, u0, v0 = column_of(axis, 0, a, b)
    return (u0, v0, u0 + 2, v0 + (2 if axis == 2 else 8))


def rects_around(axis, S, a, b):
    """small rects around bundle (a, b), clipped to the face: the bundle and a margin of 3 columns, which cuts the
    neighbouring bundles; and the bundle itself cut on every side"""
    u0, v0, u1, v1 = bundle_rect(axis, S, a, b)
    clip = lambda r: (max(r[0], 0), max(r[1], 0), min(r[2], S), min(r[3], S))
    return [clip((u0 - 3, v0 - 3, u1 + 3, v1 + 3)), (u0 + 1, v0, u1, v1), (u0, v0 + 1, u1, v1), (u0, v0, u1 - 1, v1), (u0, v0, u1, v1 - 1)]


def band_values(S):
    """{2^b - 1, 2^b, 2^b + 1} up to 2^b = S: S + 1 is the bound that selects to the end of every column"""
    return around_powers(S, top=S)


def bands(S):
    """[(lo, hi)] with lo and hi from band_values: every value is a lo and a hi at least once; hi is lo's successor two and
    seven places on, so that a band opens and closes in different words (a word along x or y has 2 levels, along z 8, and a
    comb passes a solid voxel every second level), and once the last value, S + 1"""
    v = band_values(S)
    out = []
    for i, lo in enumerate(v):
        for j in (i + 2, i + 7, len(v) - 1):
            if j < len(v) and v[j] - lo >= 2 and (lo, v[j]) not in out:
                out.append((lo, v[j]))
    return out


# ---- b. the walks, word by word -------------------------------------------------------------------------------------------

WRONG = {
    0: "the kernels as they stand",
    1: "runs has one plane fewer",
    2: "first and last have one plane fewer",
    3: "first and last are read out with the planes 8 and 9 exchanged",
    4: "add_bit's carry stops after plane 5",
    5: "last lacks the clearing term: last[p] |= s & one",
    6: "first takes s where it should take fresh",
    7: "prev is reset at every word",
    8: "runs counts s & ~seen",
    9: "SIGNED_PLANES is 11",
    10: "the band is judged after add_bit",
    11: "from_hi is initialised from lo",
    12: "for side 0 the levels of a word are taken in ascending order",
    13: "count has one plane fewer",
}


def level(axis, word, j):
    """vrc_columns.hip:51-52"""
    return (word >> np.uint32(SHIFT[axis] * j)) & np.uint32(COLUMNS[axis])


def add_bit(planes, carry, wrong=0):
    """vrc_columns.hip:102-111 on planes [P, bundles]; it leaves the loop once no column carries, which changes nothing"""
    for p in range(len(planes)):
        if (wrong == 4 and p > 5) or not carry.any():
            break
        t = planes[p] & carry
        planes[p] ^= carry
        carry = t


def read_planes(planes, bit, exchanged=False):
    """vrc_columns.hip:114-121 for every bundle: int64 [bundles]"""
    v = np.zeros(planes.shape[1], np.int64)
    for p in range(len(planes)):
        q = {8: 9, 9: 8}.get(p, p) if exchanged else p
        v |= ((planes[p] >> np.uint32(bit)) & 1).astype(np.int64) << q
    return v


def gather(words, axis, lg, a, b):
    """(the words of the walks of the bundles (a, b), shifted and masked: uint32 [bundles, steps]; their indices)"""
    idx, idx_step, shift, shift_step, mask, steps = walk_of(axis, lg, np.asarray(a, np.int64), np.asarray(b, np.int64))
    t = np.arange(steps)
    w = words[idx[:, None] + t[None, :] * idx_step]
    return (w >> (shift[:, None] + t[None, :] * shift_step).astype(np.uint32)) & np.uint32(mask), idx[:, None] + t[None, :] * idx_step


def emulate_profile(words, axis, side, a, b, wrong=0):
    """k_columns_profile (vrc_columns.hip:124-172) for the bundles (a, b) of the volume `words`, without the rect's test:
    int64 [bundles, N_COLUMNS, 4], the records of all columns of each bundle in the order of c"""
    lg = words.S.bit_length() - 2
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    walk, _ = gather(words, axis, lg, a, b)
    nbun = len(a)
    coord = COORD_PLANES - (wrong == 2)
    seen, prev = np.zeros(nbun, np.uint32), np.zeros(nbun, np.uint32)
    first, last = np.zeros((coord, nbun), np.uint32), np.zeros((coord, nbun), np.uint32)
    count, runs = np.zeros((COUNT_PLANES - (wrong == 13), nbun), np.uint32), np.zeros((COORD_PLANES - (wrong == 1), nbun), np.uint32)
    for t in range(walk.shape[1]):
        word = walk[:, t]
        if wrong == 7:
            prev = np.zeros(nbun, np.uint32)
        if not word.any() and not prev.any():
            continue                                       # empty levels change nothing: fresh = s = 0
        for j in range(LEVELS[axis]):
            s, at = level(axis, word, j), LEVELS[axis] * t + j
            before = seen
            fresh = s & ~seen
            seen = seen | s
            one = np.array([M32 if (at >> p) & 1 else 0 for p in range(coord)], np.uint32)[:, None]      # the same for every lane
            first |= (s if wrong == 6 else fresh) & one
            last[...] = (last if wrong == 5 else last & ~s) | (s & one)
            add_bit(count, s, wrong)
            add_bit(runs, s & ~before if wrong == 8 else s & ~prev, wrong)
            prev = s
    out = np.zeros((nbun, N_COLUMNS[axis], 4), np.int64)
    for c in range(N_COLUMNS[axis]):
        bit, _, _ = column_of(axis, c, 0, 0)
        least, greatest = read_planes(first, bit, wrong == 3), read_planes(last, bit, wrong == 3)
        r = np.stack([least if side else greatest, greatest if side else least, read_planes(count, bit), read_planes(runs, bit)], -1)
        out[:, c] = np.where(((seen >> np.uint32(bit)) & 1).astype(bool)[:, None], r, np.array(EMPTY_RECORD, np.int64))
    return out


def emulate_select(words, axis, side, lo, hi, of, a, b, wrong=0):
    """k_columns_select (vrc_columns.hip:175-211) for the bundles (a, b): (K as uint32 [bundles, steps] in the order of the
    words' indices, those indices).  lo and hi as vrc_columns_select hands them on (its band_lo, band_hi: at most S + 1)"""
    S = words.S
    lg = S.bit_length() - 2
    lo, hi = min(lo, S + 1), min(hi, S + 1)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    walk, index = gather(words, axis, lg, a, b)
    nbun, steps = walk.shape
    P = SIGNED_PLANES - (wrong == 9)
    solid, empty = np.uint32(M32 if of & SOLID else 0), np.uint32(M32 if of & EMPTY else 0)
    planes = lambda value: np.repeat(np.array([M32 if (-value >> p) & 1 else 0 for p in range(P)], np.uint32)[:, None], nbun, 1)
    from_lo, from_hi = planes(lo), planes(lo if wrong == 11 else hi)
    K = np.zeros((nbun, steps), np.uint32)
    L = LEVELS[axis]
    for t in (range(steps) if side else range(steps - 1, -1, -1)):
        word = walk[:, t]
        for i in range(L):
            j = i if side or wrong == 12 else L - 1 - i
            s = level(axis, word, j)
            if wrong == 10:
                add_bit(from_lo, s, wrong)
                add_bit(from_hi, s, wrong)
            in_band = ~from_lo[P - 1] & from_hi[P - 1]
            K[:, t] |= (in_band & ((s & solid) | (~s & empty)) & np.uint32(COLUMNS[axis])) << np.uint32(SHIFT[axis] * j)
            if wrong != 10:
                add_bit(from_lo, s, wrong)
                add_bit(from_hi, s, wrong)
    return K & np.uint32(walk_of(axis, lg, a, b)[4]), index                    # 4^3: what store_box_word takes is K & w.mask


def scene_bundles(sc):
    keys = sorted(sc.placed)
    return np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64)


def emulated_records(sc, side, wrong=0):
    """(the emulation's record of every programmed column in the scene's order, the number of records of unprogrammed columns
    of the programmed bundles that are not empty)"""
    a, b = scene_bundles(sc)
    rec = emulate_profile(sc.words(), sc.axis, side, a, b, wrong)
    out = np.zeros((len(sc.columns), 4), np.int64)
    stray = 0
    for k, key in enumerate(zip(a.tolist(), b.tolist())):
        for c in range(N_COLUMNS[sc.axis]):
            if c in sc.placed[key]:
                out[sc.placed[key][c]] = rec[k, c]
            else:
                stray += tuple(rec[k, c]) != EMPTY_RECORD
    return out, stray


def popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a, np.uint32).view(np.uint8)).sum())


def select_errors(sc, side, lo, hi, of, wrong=0):
    """voxels of the programmed bundles that the emulation selects and the sparse model does not, or the other way round"""
    a, b = scene_bundles(sc)
    K, index = emulate_select(sc.words(), sc.axis, side, lo, hi, of, a, b, wrong)
    return popcount(K ^ sc.selection_scene(side, lo, hi, of).words()[index])


# ---- c. the scenes of test_gpu_volume_columns.py ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def old_random(S=128):
    """test_larger_volume: the seeded random field"""
    vol = cells_model.random_set(19, cells_model.threshold_of(0.4), S)
    vol.setflags(write=False)
    return vol


def old_random_bands(S=128):
    """test_larger_volume: (direction, lo, hi, of) as it draws them"""
    rng = np.random.default_rng(S)
    out = []
    for direction in model.DIRECTIONS:
        lo = int(rng.integers(0, 5))
        out.append((direction, lo, lo + int(rng.integers(1, S // 3)), 1 + direction % 3))
    return out


def all_bundles(axis, S):
    na, nb = face_bundles(axis, S)
    a, b = np.divmod(np.arange(na * nb), nb)
    return a, b


PROFILE_SWITCHES, SELECT_SWITCHES = (1, 2, 3, 4, 5, 6, 7, 8, 13), (4, 9, 10, 11, 12)      # add_bit serves both walks


def old_random_changes(wrong, S=128):
    """(records of the six whole-face profiles, voxels of the six selections) that a wrong kernel changes on the random field
    of test_larger_volume"""
    words = Words.of_dense(old_random(S))
    records = voxels = 0
    for axis in range(3):
        a, b = all_bundles(axis, S)
        if wrong in PROFILE_SWITCHES:
            for side in (0, 1):
                records += int((emulate_profile(words, axis, side, a, b, wrong) != emulate_profile(words, axis, side, a, b)).any(-1).sum())
        if wrong in SELECT_SWITCHES:
            for direction, lo, hi, of in old_random_bands(S):
                if direction >> 1 == axis:
                    good, _ = emulate_select(words, axis, direction & 1, lo, hi, of, a, b)
                    voxels += popcount(good ^ emulate_select(words, axis, direction & 1, lo, hi, of, a, b, wrong)[0])
    return records, voxels


NOTCH_RECT = (1, 7, 5, 25)           # test_counters_of_a_full_volume: the rect it profiles; the notch is (2, 8, 4, 24) at y = S / 2


def notch_words(depth):
    """test_counters_of_a_full_volume: the full volume without the voxels (x, S / 2, z), x in 2 .. 3, z in 8 .. 23"""
    S = 1 << depth
    return Words.of_voxels(S, [(x, S // 2, z) for x in (2, 3) for z in range(8, 24)], solid=False, fill=M32)


def notch_changes(wrong, depth):
    """(records, voxels) that a wrong kernel changes on the notched full volume: the records of the bundles that NOTCH_RECT
    touches, all six directions, and the selected voxels of the test's two selections in the bundles that hold x < 6, z < 32
    (y), the only ones that differ from the plain full column"""
    S = 1 << depth
    words = notch_words(depth)
    records = voxels = 0
    for axis in range(3):
        a0, na, b0, nb = bundles(axis, *NOTCH_RECT)
        a, b = [g.reshape(-1) for g in np.meshgrid(np.arange(a0, a0 + na), np.arange(b0, b0 + nb), indexing="ij")]
        if wrong in PROFILE_SWITCHES:
            for side in (0, 1):
                records += int((emulate_profile(words, axis, side, a, b, wrong) != emulate_profile(words, axis, side, a, b)).any(-1).sum())
    if wrong in SELECT_SWITCHES:
        a, b = [g.reshape(-1) for g in np.meshgrid(np.arange(3), np.arange(4), indexing="ij")]
        for side, lo, hi, of in ((1, S - 2, S + 1, SOLID), (0, S - 2, S, BOTH)):
            good, _ = emulate_select(words, 1, side, lo, hi, of, a, b)
            voxels += popcount(good ^ emulate_select(words, 1, side, lo, hi, of, a, b, wrong)[0])
    return records, voxels
