"""The yardstick of the sight tests (include/vrc.h: vrc_sight_segments, vrc_sight_field): the rule restated in plain Python.

The walk from voxel a to voxel b sorts the crossing events t = (2k - 1) / (2 n_c) as fractions.Fraction, groups equal times
into one step, and never strides: what the device's stride may skip, this visits.  tests/test_sight_host.py holds the visited
sets against the geometry (open and closed cubes met by the segment), by a rational slab test written without the walk."""
import math
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF
THIN, TOUCH, PLAIN = 0, 1, 2
CLEAR, BLOCKED, OUTSIDE = 0, 1, 2
SIGHT_DTYPE = np.dtype([("status", "<u4"), ("at", "<u4", 3), ("before", "<u4", 3), ("reserved", "<u4")])
assert SIGHT_DTYPE.itemsize == 32


def walk(a, b, touch=False):
    """the visited voxels of the walk a -> b as a list of (x, y, z), a first and b last"""
    a, b = tuple(int(v) for v in a), tuple(int(v) for v in b)
    n = [abs(b[c] - a[c]) for c in range(3)]
    s = [1 if b[c] > a[c] else -1 for c in range(3)]
    events = sorted((Fraction(2 * k - 1, 2 * n[c]), c) for c in range(3) for k in range(1, n[c] + 1))
    cur, out, i = list(a), [a], 0
    while i < len(events):
        t, T = events[i][0], 0
        while i < len(events) and events[i][0] == t:
            T |= 1 << events[i][1]
            i += 1
        if touch and T & (T - 1):
            for sub in range(1, 7):                         # the non-empty proper subsets of T, ascending by mask
                if sub & ~T or sub == T:
                    continue
                out.append(tuple(cur[c] + (s[c] if sub >> c & 1 else 0) for c in range(3)))
        for c in range(3):
            if T >> c & 1:
                cur[c] += s[c]
        out.append(tuple(cur))
    assert tuple(cur) == b
    return out


def value_reader(field):
    """field as a function of a voxel: an (S, S, S) array, or a function already"""
    if callable(field):
        return field
    return lambda p: int(field[p[0], p[1], p[2]])


def segment(field, S, a, b, lo, hi, touch=False):
    """(status, at, before) of one segment; at and before are (0, 0, 0) for OUTSIDE"""
    if any(not 0 <= int(v) < S for v in tuple(a) + tuple(b)):
        return OUTSIDE, (0, 0, 0), (0, 0, 0)
    value = value_reader(field)
    visited = walk(a, b, touch)
    for i, p in enumerate(visited):
        if not lo <= value(p) <= hi:
            return BLOCKED, p, visited[max(i - 1, 0)]
    return CLEAR, visited[-1], visited[max(len(visited) - 2, 0)]


def sight(field, S, segments, lo, hi, touch=False):
    """the records of vrc_sight_segments for (n, 6) segments"""
    segments = np.asarray(segments, np.int64).reshape(-1, 6)
    out = np.zeros(len(segments), SIGHT_DTYPE)
    for i, seg in enumerate(segments):
        out[i] = segment(field, S, seg[:3], seg[3:], lo, hi, touch) + (0,)
    return out


def visited_arrays(segments, touch=False):
    """walk() of every segment as an (k, 3) int array: computed once, read against many fields and bands by records()"""
    return [np.array(walk(seg[:3], seg[3:], touch), np.int64) for seg in np.asarray(segments).reshape(-1, 6)]


def records(visited, D, lo, hi):
    """sight() from visited_arrays(): the same records for segments that lie inside the volume"""
    out = np.zeros(len(visited), SIGHT_DTYPE)
    for i, w in enumerate(visited):
        values = D[w[:, 0], w[:, 1], w[:, 2]]
        bad = np.flatnonzero((values < lo) | (values > hi))
        k = int(bad[0]) if len(bad) else len(w) - 1
        out[i] = (BLOCKED if len(bad) else CLEAR, w[k], w[max(k - 1, 0)], 0)
    return out


def sight_field(field, eye, radius, lo, hi, touch=False):
    """uint32 [x, y, z] of vrc_sight_field: |p - eye|^2 where p is in range and every voxel of the walk eye -> p but p
    itself is clear, NONE elsewhere, 0 at the eye"""
    S = field.shape[0]
    eye = tuple(int(v) for v in eye)
    clear = (field >= lo) & (field <= hi)
    out = np.full((S, S, S), NONE, np.uint32)
    for p in np.ndindex(S, S, S):
        d2 = sum((p[c] - eye[c]) ** 2 for c in range(3))
        if d2 == 0:
            out[p] = 0
        elif radius == 0 or d2 <= radius * radius:
            if all(clear[q] for q in walk(eye, p, touch)[:-1]):
                out[p] = d2
    return out


def field_stats(V):
    """(visible, max_d2, argmax) of a sight field: the finite values, the largest, the voxel of smallest dense index holding it"""
    finite = V != NONE
    m = int(V[finite].max())
    first = int(np.flatnonzero((V == m).reshape(-1))[0])
    S = V.shape[0]
    return int(finite.sum()), m, (first // (S * S), (first // S) % S, first % S)


def root_above(lo):
    """the least c with c * c >= lo"""
    c = math.isqrt(lo)
    return c if c * c == lo else c + 1
