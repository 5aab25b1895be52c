"""The numpy model of the column calls (include/vrc.h: vrc_columns_profile, vrc_columns_fill, vrc_columns_select): the
yardstick of test_columns_host.py, test_gpu_volume_columns.py and test_gpu_volume_columns_cpp.py.  Occupancy is dense
[x, y, z] uint8.  Written from the header's definitions: the axis is moved last (the other two keep their x < y < z order, so
the leading two indices are (u, v)), the column is turned into travel order, and the rules are np.cumsum, np.diff and argmax
along it."""
import numpy as np

REPLACE, OR, ANDNOT = 0, 1, 2
SOLID, EMPTY, BOTH = 1, 2, 3
NONE = 0xFFFFFFFF
COLUMN_DTYPE = np.dtype([("first", "<u4"), ("last", "<u4"), ("count", "<u4"), ("runs", "<u4")])
DIRECTIONS = range(6)


def travel(vol, direction):
    """(the solid voxels as bool [u, v, t] with t counting from the entry face, the axis coordinate of every t)"""
    axis, side = direction >> 1, direction & 1
    S = vol.shape[0]
    a = np.moveaxis(np.asarray(vol) != 0, axis, -1)
    coordinate = np.arange(S)
    return (a, coordinate) if side else (a[..., ::-1], coordinate[::-1])


def window(rect, S):
    return (0, 0, S, S) if rect is None else tuple(int(c) for c in rect)


def profile(vol, direction, rect=None):
    """the records of the rect's columns, (U, V) COLUMN_DTYPE"""
    S = vol.shape[0]
    a, coordinate = travel(vol, direction)
    count = a.sum(-1)
    first = coordinate[a.argmax(-1)]
    last = coordinate[S - 1 - a[..., ::-1].argmax(-1)]
    rises = np.diff(np.concatenate([np.zeros((S, S, 1), np.int8), a.astype(np.int8)], -1), axis=-1) == 1
    out = np.zeros((S, S), COLUMN_DTYPE)
    out["first"] = np.where(count > 0, first, NONE)
    out["last"] = np.where(count > 0, last, NONE)
    out["count"] = count
    out["runs"] = rises.sum(-1)
    u_lo, v_lo, u_hi, v_hi = window(rect, S)
    return np.ascontiguousarray(out[u_lo:u_hi, v_lo:v_hi])


def height_map(vol, direction, none=-1):
    p = profile(vol, direction)
    return np.where(p["count"] > 0, p["first"].astype(np.int64), none).astype(np.int32)


def thickness_map(vol, axis):
    return profile(vol, 2 * axis)["count"].copy()


def is_height_field(vol, direction, grounded=False):
    """no column has a second run; grounded: and every run reaches the exit face"""
    p = profile(vol, direction)
    exit_at = vol.shape[0] - 1 if direction & 1 else 0
    return bool((p["runs"] <= 1).all() and (not grounded or (p["last"][p["runs"] == 1] == exit_at).all()))


def apply_op(dst, bits, op):
    return bits if op == REPLACE else (dst | bits) if op == OR else (dst & (1 - bits))


def fill(vol, axis, lo, hi, rect=None, op=OR):
    """a copy of vol after vrc_columns_fill; lo, hi: an integer or an int32 map of the rect's shape"""
    S = vol.shape[0]
    u_lo, v_lo, u_hi, v_hi = window(rect, S)
    shape = (u_hi - u_lo, v_hi - v_lo)
    lo = np.clip(np.broadcast_to(np.asarray(lo, np.int64), shape), 0, S)
    hi = np.clip(np.broadcast_to(np.asarray(hi, np.int64), shape), 0, S)
    level = np.arange(S)
    span = ((level >= lo[..., None]) & (level < hi[..., None])).astype(np.uint8)
    out = np.array(vol, np.uint8)
    view = np.moveaxis(out, axis, -1)[u_lo:u_hi, v_lo:v_hi, :]
    view[...] = apply_op(view, span, op)
    return out


def before(vol, direction):
    """P(p) as int64 [x, y, z]: the solid voxels met before p along the direction"""
    axis, side = direction >> 1, direction & 1
    a, _ = travel(vol, direction)
    P = np.cumsum(a, -1) - a
    return np.moveaxis(P if side else P[..., ::-1], -1, axis)


def selection(vol, direction, lo, hi, of):
    """K as uint8 [x, y, z]"""
    solid = np.asarray(vol) != 0
    P = before(vol, direction)
    kind = (solid & bool(of & SOLID)) | (~solid & bool(of & EMPTY))
    return ((P >= lo) & (P < hi) & kind).astype(np.uint8)


def select(dst, src, direction, lo, hi, of, op=REPLACE):
    """a copy of dst after vrc_columns_select from src"""
    return apply_op(np.array(dst, np.uint8), selection(src, direction, lo, hi, of), op)


def raise_terrain(heights, depth):
    """main.cpp:65-72 as a fill of an empty volume: axis 1, lo = S/2 + 1, hi = S/2 + clamp(height, 16, S), REPLACE"""
    S = 1 << depth
    lim = np.clip(np.asarray(heights)[:S, :S].astype(np.int64), 16, S)
    return fill(np.zeros((S, S, S), np.uint8), 1, S // 2 + 1, S // 2 + lim, None, REPLACE)


def alternating(S, axis, phase=0):
    """single-voxel runs along `axis`: solid where the axis coordinate is odd (phase 1) or even (phase 0); runs == S / 2"""
    return np.ascontiguousarray(np.broadcast_to(np.moveaxis(((np.arange(S) & 1) == phase).astype(np.uint8)[None, None, :], -1, axis), (S, S, S)))
