"""The cases of tests/test_gpu_volume_rects_long.py: scenes whose runs of faces span several 32-bit words of a row, under
which the three word walks of csrc/vrc_rects.hip (run_end across the words of a row, holds_run over k0 .. k1 and the bit
beside the run in word k0 - 1 or k1 + 1, and the two carries of rect_starts) take the paths the short runs of random
fields never reach.  Beside the scenes and the records that follow from how they are made: the geometry of the passes
restated in Python from the code as it stands, each with the line it was read off; face_word, run_end, holds_run,
rect_starts, the slot scan and the height walk of k_rect_emit emulated word by word on row fields built with numpy, with
switches for ten wrong kernels; and a rectangle model that works plane by plane over the occupied planes of a list of
solid boxes, for 256^3 and 512^3 where the dense model cannot run.  tests/test_volume_rect_cases_host.py holds all of it
to its regime without a GPU.  numpy and Python integers only."""
import functools

import numpy as np

import rect_model as R
from large_volume_cases import SCAN_GROUP, scan_slots, scan_steps          # vrc_group.h: SCAN_GROUP, scan_slots and its loop, restated once

GROUP = 256                          # vrc_list.h, LIST_GROUP: lanes per workgroup
M32 = 0xFFFFFFFF
UNWRITTEN = 0xEEEEEEEE               # what a record no lane wrote reads as in Emulation.records


# ---- a. the geometry ---------------------------------------------------------------------------------------------------

def words_lg(depth):
    """vrc_rects.hip:235: log2 of the words of a row"""
    return depth - 5 if depth > 5 else 0


def field_words(depth):
    """vrc_rects.hip:237: words of one row field"""
    return 1 << (2 * depth + words_lg(depth))


def lanes_of(depth):
    """vrc_rects.hip:239"""
    return 6 * field_words(depth)


def groups_of(depth):
    """vrc_rects.hip, groups_of: workgroups of the count and emit passes = slots of the scan"""
    return (lanes_of(depth) + GROUP - 1) // GROUP


def lane_parts(L, depth):
    """vrc_rects.hip:143-149: lane -> (d, c_a, c_s, k)"""
    lgw, S1 = words_lg(depth), (1 << depth) - 1
    k = L & ((1 << lgw) - 1)
    t = L >> lgw
    cs = t & S1
    t >>= depth
    return t >> depth, t & S1, cs, k


def lane_index(d, ca, cs, k, depth):
    return ((((d << depth) + ca) << depth) + cs << words_lg(depth)) + k


def lane_of(records, S):
    """the lane that emits each packed record: (d, c_a, s0, word of r0)"""
    u = R.unpack(records)
    rows = np.arange(u.shape[0])
    a = u[:, 3] >> 1
    w = max(1, S // 32)
    return ((u[:, 3] * S + u[rows, a]) * S + u[rows, np.asarray(R.STACK)[a]]) * w + u[rows, np.asarray(R.RUN)[a]] // 32


# ---- b. the kernels, word by word ----------------------------------------------------------------------------------------

def row_fields(V):
    """what k_rect_rows leaves (vrc_rects.hip: k_rect_rows, fields_of and rows_of): the Z-rows [x][y][z bits] and behind them the Y-rows
    [x][z][y bits], w = max(1, S / 32) words a row, bits past S zero; one flat uint32 array"""
    B = np.asarray(V) != 0
    S = B.shape[0]

    def packed(rows):
        if S < 32:
            rows = np.pad(rows, ((0, 0), (0, 0), (0, 32 - S)))
        return np.packbits(rows, axis=2, bitorder="little").reshape(-1).view("<u4").astype(np.uint32)

    return np.concatenate([packed(B), packed(B.transpose(0, 2, 1))])


def face_word(fields, depth, beyond, d, ca, cs, k):
    """vrc_rects.hip:94-104 on the flat fields, index for index; k may lie beyond the row, as a wrong kernel's does.  A word
    behind the fields reads as 0"""
    a, S, lgw = d >> 1, 1 << depth, words_lg(depth)
    base = field_words(depth) if a == 2 else 0
    row, step = (ca * S + cs, S) if a == 0 else (cs * S + ca, 1)
    inside = ca + 1 < S if d & 1 else ca > 0
    beside = (row + step if d & 1 else row - step) if inside else row
    at = lambda i: int(fields[base + i]) if base + i < len(fields) else 0
    cur, nb = at((row << lgw) + k), at((beside << lgw) + k)
    return cur & ~(nb if inside else beyond) & M32


def face_words(fields, depth, closed=True):
    """face_word for every lane at once: uint32 [d][c_a][c_s][k]"""
    S, w, n = 1 << depth, 1 << words_lg(depth), field_words(depth)
    zr, yr = fields[:n].reshape(S, S, w), fields[n:2 * n].reshape(S, S, w)
    out = np.zeros((6, S, S, w), np.uint32)
    beyond = np.uint32(0 if closed else M32)
    for d in range(6):
        a = d >> 1
        field = yr if a == 2 else zr
        cur = field if a == 0 else field.transpose(1, 0, 2)               # [c_a][c_s][k]
        nb = np.empty_like(cur)
        if d & 1:
            nb[:-1], nb[-1] = cur[1:], beyond
        else:
            nb[1:], nb[0] = cur[:-1], beyond
        out[d] = cur & ~nb
    return out


def ctz(v):
    return (v & -v).bit_length() - 1


WRONG = {
    0: "the kernels as they stand",
    1: "run_end stops at the end of its own word",
    2: "run_end looks only one word ahead",
    3: "holds_run tests only the words k0 and k1",
    4: "holds_run omits bit 31 of word k0 - 1",
    5: "holds_run omits bit 0 of word k1 + 1",
    6: "holds_run drops the r1 < S guard and reads the first word of the next row",
    7: "rect_starts drops carry",
    8: "rect_starts drops pcarry",
    9: "the emit's height walk stops at the first following row",
    10: "the scan starts each step from zero",
}


class Emulation:
    """k_rect_count<false>, k_scan_slots and k_rect_emit<FACES> on row fields; wrong: one of WRONG.  The counters say which
    paths the field took: run_end calls by the words they went on to (loops), holds_run's visits of a word strictly between
    k0 and k1 and the calls decided there, the reads of the bit beside a word-aligned end, and the calls with r1 == S"""

    def __init__(self, fields, depth, closed=True, wrong=0):
        self.fields, self.depth, self.closed, self.wrong = fields, depth, closed, wrong
        self.S, self.lgw, self.w = 1 << depth, words_lg(depth), 1 << words_lg(depth)
        self.beyond = 0 if closed else M32
        self.faces = face_words(fields, depth, closed).reshape(-1)
        self.f = self.faces.tolist()
        self.loops = [0, 0, 0, 0]             # run_end calls that went on to 0, 1, 2, 3 or more further words
        self.holds_calls = self.middle_visits = self.middle_false = 0
        self.low_reads = self.low_false = self.high_reads = self.high_false = self.row_end_calls = 0
        self._starts = None

    def word(self, base, k):
        """the faces of word k of the row whose word 0 is lane `base`"""
        if 0 <= k < self.w:
            return self.f[base + k]
        d, ca, cs, _ = lane_parts(base, self.depth)
        return face_word(self.fields, self.depth, self.beyond, d, ca, cs, k)

    def run_end(self, base, k, m, b):
        """vrc_rects.hip:107-115"""
        inv = ~m & (M32 << b) & M32
        loops = 0
        while not inv:
            if self.wrong == 1 or (self.wrong == 2 and loops == 1):
                break
            k += 1
            if k == self.w:
                self.loops[min(loops, 3)] += 1
                return 32 * k
            inv = ~self.f[base + k] & M32
            loops += 1
        self.loops[min(loops, 3)] += 1
        return 32 * k + ctz(inv) if inv else 32 * (k + 1)

    def holds_run(self, base, r0, r1):
        """vrc_rects.hip:118-133; base: the lane of word 0 of the row asked"""
        k0, k1 = r0 >> 5, (r1 - 1) >> 5
        self.holds_calls += 1
        self.row_end_calls += r1 == self.S and not r1 & 31
        for k in range(k0, k1 + 1):
            middle = k0 < k < k1
            if middle and self.wrong == 3:
                continue
            w = self.f[base + k]
            lo = r0 & 31 if k == k0 else 0
            hi = (r1 - 1) & 31 if k == k1 else 31
            mask = (M32 << lo) & (M32 >> (31 - hi)) & M32
            self.middle_visits += middle
            if (w & mask) != mask:
                self.middle_false += middle
                return False
            if lo and (w >> (lo - 1)) & 1:
                return False
            if hi < 31 and (w >> (hi + 1)) & 1:
                return False
        if not r0 & 31 and r0 and self.wrong != 4:
            self.low_reads += 1
            if self.f[base + k0 - 1] >> 31:
                self.low_false += 1
                return False
        if not r1 & 31 and (r1 < self.S or self.wrong == 6) and self.wrong != 5:
            self.high_reads += 1
            if self.word(base, k1 + 1) & 1:
                self.high_false += 1
                return False
        return True

    def rect_starts(self, L):
        """vrc_rects.hip:141-164 for a lane whose word has faces"""
        f, w = self.f, self.w
        m = f[L]
        k = L & (w - 1)
        cs = (L >> self.lgw) & (self.S - 1)
        carry = f[L - 1] >> 31 if k and self.wrong != 7 else 0
        starts = m & ~((m << 1) | carry) & M32
        if not cs:
            return starts
        pm = f[L - w]
        pcarry = f[L - w - 1] >> 31 if k and self.wrong != 8 else 0
        rs = starts & ~(pm & ~((pm << 1) | pcarry))
        s = starts & ~rs
        while s:
            b = ctz(s)
            if not self.holds_run(L - k - w, 32 * k + b, self.run_end(L - k, k, m, b)):
                rs |= 1 << b
            s &= s - 1
        return rs

    def starts(self):
        """[(lane, its rectangle starts)] of the lanes that have any, ascending"""
        if self._starts is None:
            self._starts = [(L, rs) for L, rs in ((int(L), self.rect_starts(int(L))) for L in np.flatnonzero(self.faces)) if rs]
        return self._starts

    def slots(self):
        """(the slots after k_scan_slots, the total it reports)"""
        counts = np.zeros(groups_of(self.depth), np.int64)
        for L, rs in self.starts():
            counts[L // GROUP] += bin(rs).count("1")
        return scan_slots(counts, carry=self.wrong != 10)

    def records(self, first=0, capacity=None):
        """the window [first, first + capacity) of k_rect_emit's records, capacity=None: up to the total the scan reports; a
        record that no lane writes reads as UNWRITTEN"""
        offsets, total = self.slots()
        edges = np.append(offsets, total)
        n = max(0, total - first) if capacity is None else max(0, min(capacity, total - first))
        win_end = first + n
        out = np.full((n, 4), UNWRITTEN, np.uint32)
        S, w, wrong = self.S, self.w, self.wrong
        idx, group = 0, -1
        for L, rs in self.starts():
            g = L // GROUP
            if g != group:
                group, idx = g, int(edges[g])
                leaves = edges[g] == edges[g + 1] or edges[g + 1] <= first or edges[g] >= win_end     # vrc_list.h, list_window
            if leaves:
                continue
            d, ca, cs, k = lane_parts(L, self.depth)
            a = d >> 1
            m = self.f[L]
            while rs:
                if first <= idx < win_end:
                    b = ctz(rs)
                    r0, r1 = 32 * k + b, self.run_end(L - k, k, m, b)
                    ns = 1
                    while cs + ns < S and self.holds_run(L - k + ns * w, r0, r1):
                        ns += 1
                        if wrong == 9:
                            break
                    x, y, z = (ca, cs, r0) if a == 0 else (cs, ca, r0) if a == 1 else (cs, r0, ca)
                    out[idx - first] = (x, y, z, d | ((r1 - r0 - 1) << 8) | ((ns - 1) << 20))
                rs &= rs - 1
                idx += 1
        return out


def emulated(V, closed=True, wrong=0):
    V = np.asarray(V)
    return Emulation(row_fields(V), int(V.shape[0]).bit_length() - 1, closed, wrong).records()


# ---- c. the sparse model -----------------------------------------------------------------------------------------------

class BoxPlanes:
    """the planes of a union of solid boxes (n, 6) x0 y0 z0 x1 y1 z1 in S^3, rasterised when asked for"""

    def __init__(self, boxes, S):
        b = np.asarray(boxes, np.int64).reshape(-1, 6)
        self.S, self.lo, self.hi = S, b[:, :3], np.minimum(b[:, 3:], S)
        self.lo, self.hi = self.lo[(self.lo < self.hi).all(axis=1)], self.hi[(self.lo < self.hi).all(axis=1)]
        self._sel, self._plane = {}, {}

    def occupied(self, a):
        mark = np.zeros(self.S + 1, np.int64)
        np.add.at(mark, self.lo[:, a], 1)
        np.add.at(mark, self.hi[:, a], -1)
        return np.flatnonzero(np.cumsum(mark)[:self.S] > 0).tolist()

    def key(self, a, c):
        """equal for two planes of an axis iff the same boxes cover them"""
        if (a, c) not in self._sel:
            self._sel[a, c] = np.flatnonzero((self.lo[:, a] <= c) & (c < self.hi[:, a]))
        return a, self._sel[a, c].tobytes()

    def plane(self, a, c):
        """bool [c_s, c_r]: the other two axes in ascending order"""
        key = self.key(a, c)
        if key not in self._plane:
            sel, (s, r) = self._sel[a, c], [x for x in range(3) if x != a]
            out = np.zeros((self.S, self.S), bool)
            if len(sel):
                s0, r0, s1, r1 = self.lo[sel, s], self.lo[sel, r], self.hi[sel, s], self.hi[sel, r]
                os, or_, ns, nr = s0.min(), r0.min(), s1.max() - s0.min(), r1.max() - r0.min()       # the boxes' bounds: nothing lies outside
                D = np.zeros((ns + 1, nr + 1), np.int32)
                for rows, cols, sign in ((s0, r0, 1), (s0, r1, -1), (s1, r0, -1), (s1, r1, 1)):
                    np.add.at(D, (rows - os, cols - or_), sign)
                out[os:os + ns, or_:or_ + nr] = D.cumsum(axis=0).cumsum(axis=1)[:ns, :nr] > 0
            self._plane[key] = out
        return self._plane[key]


class DensePlanes:
    """the planes of a dense field V[x, y, z]"""

    def __init__(self, V):
        self.V, self.S = np.asarray(V) != 0, V.shape[0]

    def occupied(self, a):
        return np.flatnonzero(self.V.any(axis=tuple(x for x in range(3) if x != a))).tolist()

    def key(self, a, c):
        return a, c

    def plane(self, a, c):
        return self.V.take(c, axis=a)


def plane_rects_2d(M):
    """the rectangles of one plane M[c_s, c_r] bool: (n, 4) int64 s0 r0 nr ns ordered by (s0, r0)"""
    rows, cols = np.flatnonzero(M.any(axis=1)), np.flatnonzero(M.any(axis=0))
    if not len(rows):
        return np.zeros((0, 4), np.int64)
    # inside the bounds of what is set: the rows and cells outside hold no run and end every walk
    origin = np.array([rows[0], cols[0], 0, 0])
    M = M[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
    S = max(M.shape)
    P = np.pad(M, ((0, 0), (1, 1)))
    begin, end = np.argwhere(P[:, 1:-1] & ~P[:, :-2]), np.argwhere(P[:, 1:-1] & ~P[:, 2:])
    cs, r0, r1 = begin[:, 0], begin[:, 1], end[:, 1] + 1
    runs = (cs * (S + 1) + r0) * (S + 1) + r1                           # ascending: rows, then the runs of a row
    held = lambda keys: runs[np.minimum(np.searchsorted(runs, keys), len(runs) - 1)] == keys
    first = (cs == 0) | ~held(runs - (S + 1) ** 2)                      # the same run one row before
    cs, r0, r1, runs = cs[first], r0[first], r1[first], runs[first]
    # the heights by the cells themselves, not by keys: C[:, j] = set cells before column j of the padded plane
    C = np.concatenate([np.zeros((M.shape[0], 1), np.int64), np.cumsum(P, axis=1, dtype=np.int64)], axis=1)
    ns = np.ones(len(cs), np.int64)
    alive = np.arange(len(cs))
    while len(alive):
        alive = alive[cs[alive] + ns[alive] < M.shape[0]]
        row, a0, a1 = cs[alive] + ns[alive], r0[alive], r1[alive]
        alive = alive[(C[row, a1 + 1] - C[row, a0 + 1] == a1 - a0) & ~P[row, a0] & ~P[row, a1 + 1]]
        ns[alive] += 1
    return np.stack([cs, r0, r1 - r0, ns], axis=1) + origin


def sparse_rects(planes, closed=True):
    """the packed records of rect_model.rects from a plane provider (BoxPlanes, DensePlanes), over the occupied planes only;
    planes covered by the same boxes are worked once"""
    S, out, done = planes.S, [], {}
    for d in range(6):
        a, side = d >> 1, d & 1
        s, r = R.STACK[a], R.RUN[a]
        for c in planes.occupied(a):
            nb = c + 1 if side else c - 1
            if 0 <= nb < S:
                key = (planes.key(a, c), planes.key(a, nb))
                if key[0] == key[1]:
                    continue
            elif closed:
                key = (planes.key(a, c), None)
            else:
                continue
            if key not in done:
                M = planes.plane(a, c)
                done[key] = plane_rects_2d(M & ~planes.plane(a, nb) if key[1] else M)
            p = done[key]
            xyz = np.zeros((p.shape[0], 3), np.int64)
            xyz[:, a], xyz[:, s], xyz[:, r] = c, p[:, 0], p[:, 1]
            out.append(R.pack(xyz, np.full(p.shape[0], d), p[:, 2], p[:, 3]))
    return np.concatenate(out) if out else np.zeros((0, 4), np.uint32)


def dense_of_boxes(boxes, S):
    V = np.zeros((S, S, S), np.uint8)
    for x0, y0, z0, x1, y1, z1 in np.asarray(boxes, np.int64).reshape(-1, 6).tolist():
        V[x0:x1, y0:y1, z0:z1] = 1
    return V


# ---- d. the scenes -----------------------------------------------------------------------------------------------------

class Scene:
    """name, depth, S, axis (of the sheets' faces, or None), boxes (n, 6) or None, and for the sheet scenes `expected`: the
    packed records of the directions 2 axis and 2 axis + 1 that follow from the construction, in canonical order.  dense():
    the field V[x, y, z] (up to 256^3)"""

    def __init__(self, name, depth, axis=None, boxes=None, expected=None, field=None):
        self.name, self.depth, self.S, self.axis, self.expected, self._field = name, depth, 1 << depth, axis, expected, field
        self.boxes = None if boxes is None else np.asarray(boxes, np.uint32).reshape(-1, 6)

    def dense(self):
        if self._field is None:
            self._field = dense_of_boxes(self.boxes, self.S)
            self._field.setflags(write=False)
        return self._field

    def planes(self):
        return BoxPlanes(self.boxes, self.S) if self.boxes is not None else DensePlanes(self._field)


class Sheets:
    """rows of runs on one-voxel-thick sheets normal to `axis`, at the odd planes 1, 3, .. so that both sides of a sheet are
    exposed: add(plane, s0, s1, r0, r1) sets the rows [s0, s1) of a sheet to hold [r0, r1); expect(plane, s0, r0, nr, ns)
    notes a rectangle of both of its face directions"""

    def __init__(self, S, axis):
        self.S, self.axis, self.boxes, self.want = S, axis, [], []
        self.s, self.r = R.STACK[axis], R.RUN[axis]

    def add(self, plane, s0, s1, r0, r1):
        assert 0 < plane < self.S - 1 and plane & 1 and 0 <= s0 < s1 <= self.S and 0 <= r0 < r1 <= self.S
        lo, hi = [0, 0, 0], [0, 0, 0]
        lo[self.axis], hi[self.axis] = plane, plane + 1
        lo[self.s], hi[self.s] = s0, s1
        lo[self.r], hi[self.r] = r0, r1
        self.boxes.append(lo + hi)

    def expect(self, plane, s0, r0, nr, ns):
        self.want.append((plane, s0, r0, nr, ns))

    def expected(self):
        p = np.array(sorted(self.want), np.int64).reshape(-1, 5)
        xyz = np.zeros((len(p), 3), np.int64)
        xyz[:, self.axis], xyz[:, self.s], xyz[:, self.r] = p[:, 0], p[:, 1], p[:, 2]
        return np.concatenate([R.pack(xyz, np.full(len(p), 2 * self.axis + side), p[:, 3], p[:, 4]) for side in (0, 1)])

    def scene(self, name, depth):
        return Scene(name, depth, self.axis, self.boxes, self.expected())


def sheet_records(records, axis):
    """the records of the two face directions of sheets normal to `axis`"""
    records = np.asarray(records)
    return records[(records[:, 3] & 0xff) >> 1 == axis]


def pair_starts(S):
    """r0 of row A: the first two words' edges and their neighbours; from 256 up also the middle word's and the last word"""
    r0 = [0, 1, 31, 32, 33, 63, 64]
    if S > 128:
        r0 += [S // 2 - 1, S // 2, S // 2 + 1, S - 32]
    return r0


def pair_ends(S):
    """r1 of row A: every word edge and its neighbours up to S"""
    return sorted({e + o for e in range(32, S + 1, 32) for o in (-1, 0, 1) if e + o <= S})


def pair_variants(S, r0, r1):
    """[(what, the runs of row B)] for row A = [r0, r1), r1 - r0 >= 2: identical, one cell longer or shorter at either end, and
    A with a single hole at bit 0, 15 or 31 of a word the run covers, strictly inside the run -- of every such word up to
    four words a row, of the first two, the middle and the last one beyond"""
    out = [("same", [(r0, r1)]), ("short-lo", [(r0 + 1, r1)]), ("short-hi", [(r0, r1 - 1)])]
    if r0 > 0:
        out.append(("long-lo", [(r0 - 1, r1)]))
    if r1 < S:
        out.append(("long-hi", [(r0, r1 + 1)]))
    k0, k1 = r0 >> 5, (r1 - 1) >> 5
    words = range(k0, k1 + 1) if S <= 128 else sorted({k0, min(k0 + 1, k1), (k0 + k1) // 2, k1})
    for k in words:
        for bit in (0, 15, 31):
            p = 32 * k + bit
            if r0 < p < r1 - 1:
                out.append(("hole", [(r0, p), (p + 1, r1)]))
    return out


@functools.lru_cache(maxsize=None)
def pair_table(depth, axis):
    """pairs of consecutive rows (A, B) and an empty row, S // 3 pairs a sheet, as boxes; expected: one record with ns = 2
    for the identical pair, otherwise A's run and B's runs apart"""
    S = 1 << depth
    sheets = Sheets(S, axis)
    n = 0
    for r0 in pair_starts(S):
        for r1 in pair_ends(S):
            if r1 - r0 < 2:
                continue
            for what, runs in pair_variants(S, r0, r1):
                plane, row = 1 + 2 * (n // (S // 3)), 3 * (n % (S // 3))
                n += 1
                sheets.add(plane, row, row + 1, r0, r1)
                for b0, b1 in runs:
                    sheets.add(plane, row + 1, row + 2, b0, b1)
                if what == "same":
                    sheets.expect(plane, row, r0, r1 - r0, 2)
                else:
                    sheets.expect(plane, row, r0, r1 - r0, 1)
                    for b0, b1 in runs:
                        sheets.expect(plane, row + 1, b0, b1 - b0, 1)
    scene = sheets.scene("pairs %s %d" % ("xyz"[axis], S), depth)
    scene.pairs = n
    return scene


@functools.lru_cache(maxsize=None)
def stacks(depth, axis):
    """identical multi-word runs stacked 1, 2 and 3 high with empty rows between, two stacks of different runs touching, a
    stack of height S, and one of height S interrupted at row 5 S / 8 - 3 by a row that lacks one bit of the last word but
    one"""
    S = 1 << depth
    sheets = Sheets(S, axis)
    a0, a1 = 7, S - 23                                      # a run over every word of the row
    row = 0
    for h in (1, 2, 3):
        sheets.add(1, row, row + h, a0, a1)
        sheets.expect(1, row, a0, a1 - a0, h)
        row += h + 1
    sheets.add(1, row, row + 3, 32, S)                      # word-aligned at both ends, and one that ends a cell earlier on it
    sheets.add(1, row + 3, row + 5, 32, S - 1)
    sheets.expect(1, row, 32, S - 32, 3)
    sheets.expect(1, row + 3, 32, S - 33, 2)
    sheets.add(3, 0, S, 5, S - 27)
    sheets.expect(3, 0, 5, S - 32, S)
    cut, hole = 5 * S // 8 - 3, S - 64 + 7
    sheets.add(5, 0, cut, 32, S)
    sheets.add(5, cut, cut + 1, 32, hole)
    sheets.add(5, cut, cut + 1, hole + 1, S)
    sheets.add(5, cut + 1, S, 32, S)
    sheets.expect(5, 0, 32, S - 32, cut)
    sheets.expect(5, cut, 32, hole - 32, 1)
    sheets.expect(5, cut, hole + 1, S - hole - 1, 1)
    sheets.expect(5, cut + 1, 32, S - 32, S - cut - 1)
    return sheets.scene("stacks %s %d" % ("xyz"[axis], S), depth)


@functools.lru_cache(maxsize=None)
def blocky(depth, run_axis, seed=7):
    """a coarse random field (half of its cells solid) whose cells are 2 x 2 x 40 voxels, the 40 along `run_axis` (2: the
    rows of the x and y faces; 1: those of the z faces), so that runs of 40, 80, 120, .. cells begin at multiples of 40, off
    the word grid; then one voxel in 5000 cleared and one in 10000 set: long runs whose neighbouring rows are now identical,
    now differ in one far cell.  The scene keeps its making (cells as boxes, holes, specks) for fillBoxes and setVoxels"""
    S = 1 << depth
    rng = np.random.default_rng(1000 * depth + 10 * run_axis + seed)
    shape, size = [S // 2, S // 2, S // 2], np.array([2, 2, 2])
    shape[run_axis], size[run_axis] = -(-S // 40), 40
    lo = np.argwhere(rng.random(shape) < 0.5) * size
    scene = Scene("blocky %s %d" % ("xyz"[run_axis], S), depth)
    scene.cells = np.concatenate([lo, np.minimum(lo + size, S)], axis=1).astype(np.uint32)
    scene.holes = rng.integers(0, S, (S ** 3 // 5000, 3)).astype(np.uint32)
    scene.specks = rng.integers(0, S, (S ** 3 // 10000, 3)).astype(np.uint32)
    V = dense_of_boxes(scene.cells, S)
    V[tuple(scene.holes.T.astype(np.int64))] = 0
    V[tuple(scene.specks.T.astype(np.int64))] = 1
    V.setflags(write=False)
    scene._field = V
    return scene


def full_volume(depth):
    S = 1 << depth
    want = R.pack([[0, 0, 0], [S - 1, 0, 0], [0, 0, 0], [0, S - 1, 0], [0, 0, 0], [0, 0, S - 1]], np.arange(6), np.full(6, S), np.full(6, S))
    return Scene("full %d" % S, depth, boxes=[[0, 0, 0, S, S, S]], expected=want)


def slab(depth, axis, side):
    """the one-voxel slab on a wall of the volume"""
    S = 1 << depth
    lo, hi = [0, 0, 0], [S, S, S]
    lo[axis], hi[axis] = (S - 1, S) if side else (0, 1)
    return Scene("slab %s%d %d" % ("xyz"[axis], side, S), depth, boxes=[lo + hi])


def small_constructed(S=16):
    """the constructed pairs of tests/test_gpu_volume_rects.py at the scale of a row shorter than a word: h = S / 2"""
    h = S // 2
    V = np.zeros((S, S, S), np.uint8)
    V[3, 7, 0:h], V[4, 7, 0:h + 1] = 1, 1
    V[9, 7, 1:h + 4], V[10, 7, 0:h + 4] = 1, 1
    V[12, 7, 5:11], V[13, 7, 5:11], V[14, 7, 5:12] = 1, 1, 1
    V[0, 7, :], V[1, 7, :] = 1, 1
    V[1, 7, h + 3] = 0
    V[6, 0:h, 14], V[7, 0:h + 1, 14] = 1, 1
    V[11, :, 14], V[12, :, 14] = 1, 1
    V[12, h, 14] = 0
    return V


# the +y records (x y z d nr ns) of small_constructed(16) on the sheet y = 7, the columns at z = 14 that cross it included
SMALL_UP = [[0, 7, 0, 3, 16, 1], [1, 7, 0, 3, 11, 1], [1, 7, 12, 3, 4, 1], [3, 7, 0, 3, 8, 1], [4, 7, 0, 3, 9, 1], [6, 7, 14, 3, 1, 1],
            [9, 7, 1, 3, 11, 1], [10, 7, 0, 3, 12, 1], [12, 7, 5, 3, 6, 2], [12, 7, 14, 3, 1, 1], [14, 7, 5, 3, 7, 1]]
