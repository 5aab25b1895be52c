"""The numpy model of vrc_volume_stamp_affine (include/vrc.h), vectorised in int64, and the Python mirrors of
affine_signed_permutation and of vrc_affine_place's formulas: the yardstick of tests/test_gpu_volume_stamp.py, itself held
against the definition taken literally in tests/test_volume_stamp_host.py.  Volumes are dense uint8 [x, y, z] arrays of
0 / 1, the layout of vrc_volume_download."""
import itertools

import numpy as np

REPLACE, OR, ANDNOT = 0, 1, 2
M_LIMIT, T_LIMIT = 1 << 20, 1 << 40
ONE = 65536
IDENTITY = ([ONE, 0, 0, 0, ONE, 0, 0, 0, ONE], [0, 0, 0])


def clip_box(S, lo, hi):
    """the box clipped to a volume of S^3 as unsigned 32-bit bounds, None when nothing is left"""
    lo = [int(v) & 0xFFFFFFFF for v in lo]
    hi = [min(int(v) & 0xFFFFFFFF, S) for v in hi]
    return None if any(l >= h for l, h in zip(lo, hi)) else (lo, hi)


def source_bits(src, m, t, lo, hi):
    """the source bit of every voxel of the (clipped, non-empty) box, as a uint8 array of the box's shape"""
    Ss = src.shape[0]
    m = np.asarray([int(v) for v in m], np.int64).reshape(3, 3)
    t = np.asarray([int(v) for v in t], np.int64)
    assert np.abs(m).max() <= M_LIMIT and np.abs(t).max() <= T_LIMIT        # inside these |s| < 2^41: int64 is exact
    c = [2 * np.arange(lo[a], hi[a], dtype=np.int64) + 1 for a in range(3)]
    q = []
    for a in range(3):
        s = m[a, 0] * c[0][:, None, None] + m[a, 1] * c[1][None, :, None] + m[a, 2] * c[2][None, None, :] + t[a]
        q.append(s >> 17)                                                    # arithmetic shift = floor
    inside = (q[0] >= 0) & (q[0] < Ss) & (q[1] >= 0) & (q[1] < Ss) & (q[2] >= 0) & (q[2] < Ss)
    bits = np.zeros(inside.shape, np.uint8)
    bits[inside] = src[q[0][inside], q[1][inside], q[2][inside]] != 0
    return bits


def stamp(dst, src, m, t, lo=None, hi=None, op=REPLACE):
    """a copy of dst with the box [lo, hi) (the whole volume by default) stamped from src through the inverse map (m, t)"""
    Sd = dst.shape[0]
    out = (np.asarray(dst) != 0).astype(np.uint8)
    box = clip_box(Sd, (0, 0, 0) if lo is None else lo, (Sd, Sd, Sd) if hi is None else hi)
    if box is None:
        return out
    lo, hi = box
    bits = source_bits(src, m, t, lo, hi)
    view = out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    if op == REPLACE:
        view[...] = bits
    elif op == OR:
        view |= bits
    elif op == ANDNOT:
        view &= 1 - bits
    else:
        raise ValueError(op)
    return out


def aimed_maps(rng, Ss, Sd, count):
    """random maps that send the destination's centre near the source's: general matrices up to three source voxels per
    destination voxel, so shears, mirrorings and partial coverage all occur"""
    maps = []
    for _ in range(count):
        m = [int(v) for v in rng.integers(-3 * ONE, 3 * ONE + 1, 9)]
        centre = rng.integers(Ss // 4, Ss - Ss // 4, 3)
        t = [int(centre[a]) * (1 << 17) + int(rng.integers(0, 1 << 17)) - sum(m[3 * a + b] for b in range(3)) * Sd for a in range(3)]
        maps.append((m, t))
    return maps


def signed_permutation(perm, flip, size):
    """(m, t) of q_a = p[perm[a]], or size-1 - p[perm[a]] where flip[a] is set"""
    m, t = [0] * 9, [0] * 3
    for a in range(3):
        m[3 * a + perm[a]] = -ONE if flip[a] else ONE
        t[a] = (size << 17) if flip[a] else 0
    return m, t


def all_signed_permutations():
    return [(perm, flip) for perm in itertools.permutations(range(3)) for flip in itertools.product((0, 1), repeat=3)]


def permuted(src, perm, flip):
    """out[p] = src[q] with q_a = p[perm[a]] (mirrored where flip[a]), by np.flip and np.transpose alone"""
    f = src
    for a in range(3):
        if flip[a]:
            f = np.flip(f, axis=a)
    # out[p0, p1, p2] = f[p[perm[0]], p[perm[1]], p[perm[2]]]: axis a of f becomes axis perm[a] of out
    return np.ascontiguousarray(np.transpose(f, np.argsort(perm)))


def place(rot, scale, src_pivot, dst_pivot, src_depth, dst_depth):
    """vrc_affine_place's formulas in Python doubles, operation for operation: (m, t, lo, hi).  rot is make_rotation's
    layout (columns), so the forward rotation's R[r][c] is rot[3c + r] and the inverse's row a, column b is rot[3a + b]."""
    rot = [float(np.float32(v)) for v in np.asarray(rot).reshape(9)]
    scale = float(np.float32(scale))
    sp = [float(np.float32(v)) for v in src_pivot]
    dp = [float(np.float32(v)) for v in dst_pivot]
    m, t = [0] * 9, [0] * 3
    for a in range(3):
        row = [float(np.rint(65536.0 * rot[3 * a + b] / scale)) for b in range(3)]
        total = (row[0] * 2.0 * dp[0] + row[1] * 2.0 * dp[1]) + row[2] * 2.0 * dp[2]
        m[3 * a:3 * a + 3] = [int(v) for v in row]
        t[a] = int(np.rint(131072.0 * sp[a] - total))
    Ss, Sd = float(1 << src_depth), float(1 << dst_depth)
    lo, hi = [0] * 3, [0] * 3
    for r in range(3):
        xs = []
        for corner in range(8):
            x = dp[r]
            for c in range(3):
                x += scale * rot[3 * c + r] * ((Ss if (corner >> c) & 1 else 0.0) - sp[c])
            xs.append(x)
        lo[r] = int(max(np.floor(min(xs)) - 2.0, 0.0))
        hi[r] = int(min(np.ceil(max(xs)) + 2.0, Sd))
    if any(l >= h for l, h in zip(lo, hi)):
        lo, hi = [0] * 3, [0] * 3
    return m, t, lo, hi


def rotation(axis, angle):
    """a rotation about one coordinate axis in make_rotation's layout (columns), float32"""
    c, s = np.cos(angle), np.sin(angle)
    u, v = (axis + 1) % 3, (axis + 2) % 3
    R = np.eye(3)
    R[u, u], R[u, v], R[v, u], R[v, v] = c, -s, s, c
    return np.ascontiguousarray(R.T, np.float32).reshape(9)          # rot[3c + r] = R[r][c]


def compose(rot_a, rot_b):
    """R_a R_b, both in the column layout"""
    A, B = np.asarray(rot_a, np.float64).reshape(3, 3).T, np.asarray(rot_b, np.float64).reshape(3, 3).T
    return np.ascontiguousarray((A @ B).T, np.float32).reshape(9)
