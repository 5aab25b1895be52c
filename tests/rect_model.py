"""numpy restatement of the rule of vrc_extract_rects (include/vrc.h), the yardstick of the rectangle tests: the
exposed faces of surface_model.faces merged into rectangles by the identical-run rule, their canonical order
(d, c_a, s0, r0), their packed records and their two triangles each.  tests/test_volume_rects_host.py holds it against a
per-cell restatement of the definition and, through the voxeliser's model, against the round trip."""
import numpy as np

import surface_model as F

UNIT = F.UNIT
STACK = (1, 0, 0)           # per axis a: the stack axis s and the run axis r, the other two axes with s < r
RUN = (2, 2, 1)


def face_masks(V, closed=True):
    """(6, S, S, S) bool: mask[d, x, y, z] = face d of voxel (x, y, z) is exposed, from surface_model.faces"""
    S = np.asarray(V).shape[0]
    f = F.faces(V, closed).astype(np.int64)
    mask = np.zeros((6, S, S, S), bool)
    mask[f[:, 3], f[:, 0], f[:, 1], f[:, 2]] = True
    return mask


def pack(xyz, d, nr, ns):
    """(n, 4) uint32 records: x y z and d | (nr - 1) << 8 | (ns - 1) << 20"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    w = np.asarray(d, np.int64) | ((np.asarray(nr, np.int64) - 1) << 8) | ((np.asarray(ns, np.int64) - 1) << 20)
    return np.concatenate([xyz, w.reshape(-1, 1)], axis=1).astype(np.uint32)


def unpack(records):
    """(n, 6) int64 x y z d nr ns"""
    r = np.asarray(records, np.int64).reshape(-1, 4)
    w = r[:, 3]
    return np.stack([r[:, 0], r[:, 1], r[:, 2], w & 0xff, ((w >> 8) & 0x3ff) + 1, ((w >> 20) & 0x3ff) + 1], axis=1)


def plane_rects(M):
    """the rectangles of one direction: M[c_a, c_s, c_r] bool -> (n, 5) int64 c_a s0 r0 nr ns ordered by (c_a, s0, r0)"""
    S = M.shape[0]
    P = np.pad(M, ((0, 0), (0, 0), (1, 1)))
    begin = np.argwhere(P[:, :, 1:-1] & ~P[:, :, :-2])                # run starts, in the order (c_a, c_s, r0)
    end = np.argwhere(P[:, :, 1:-1] & ~P[:, :, 2:])                   # the last cell of each run, in the same order
    ca, cs, r0, r1 = begin[:, 0], begin[:, 1], begin[:, 2], end[:, 2] + 1
    key = lambda row: ((ca * (S + 1) + row) * (S + 1) + r0) * (S + 1) + r1       # a run of row `row`; row S holds none
    runs = key(cs)
    first = ~np.isin(key(cs - 1), runs) | (cs == 0)                   # the row before does not hold the identical run
    ca, cs, r0, r1 = ca[first], cs[first], r0[first], r1[first]
    ns = np.ones(ca.shape[0], np.int64)
    alive = np.ones(ca.shape[0], bool)
    while alive.any():
        alive &= (cs + ns < S) & np.isin(key(cs + ns), runs)
        ns += alive
    return np.stack([ca, cs, r0, r1 - r0, ns], axis=1)


def rects(V, closed=True):
    """the rectangles of the dense field V[x, y, z] as packed (n, 4) uint32 records in the canonical order"""
    mask = face_masks(V, closed)
    out = []
    for d in range(6):
        a = d >> 1
        s, r = STACK[a], RUN[a]
        p = plane_rects(mask[d].transpose(a, s, r))
        xyz = np.zeros((p.shape[0], 3), np.int64)
        xyz[:, a], xyz[:, s], xyz[:, r] = p[:, 0], p[:, 1], p[:, 2]
        out.append(pack(xyz, np.full(p.shape[0], d), p[:, 3], p[:, 4]))
    return np.concatenate(out)


def ordered(records):
    """packed records in the canonical order (d, c_a, s0, r0)"""
    records = np.asarray(records, np.uint32).reshape(-1, 4)
    u = unpack(records)
    rows = np.arange(u.shape[0])
    a = u[:, 3] >> 1
    s, r = np.asarray(STACK)[a], np.asarray(RUN)[a]
    return records[np.lexsort((u[rows, r], u[rows, s], u[rows, a], u[:, 3]))]


def triangles(records):
    """(2n, 9) int32: the two triangles of each rectangle, 64 units per voxel, counter-clockwise seen from outside"""
    f = unpack(records)
    n = f.shape[0]
    rows = np.arange(n)
    d = f[:, 3]
    a, side = d >> 1, d & 1
    u, v = (a + 1) % 3, (a + 2) % 3
    e = np.ones((n, 3), np.int64)
    e[rows, np.asarray(RUN)[a]] = f[:, 4]
    e[rows, np.asarray(STACK)[a]] = f[:, 5]
    q = np.zeros((n, 4, 3), np.int64)
    for k, (du, dv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
        q[rows, k, a] = UNIT * (f[rows, a] + side)
        q[rows, k, u] = UNIT * (f[rows, u] + du * e[rows, u])
        q[rows, k, v] = UNIT * (f[rows, v] + dv * e[rows, v])
    out_plus = q[:, [0, 1, 2, 0, 2, 3], :]
    out_minus = q[:, [0, 2, 1, 0, 3, 2], :]
    return np.where((side == 1)[:, None, None], out_plus, out_minus).reshape(2 * n, 9).astype(np.int32)


def direction_counts(records):
    return np.bincount(np.asarray(records, np.int64).reshape(-1, 4)[:, 3] & 0xff, minlength=6).astype(np.uint64)


def cover(records, S):
    """(6, S, S, S) int: how many rectangles hold face d of voxel (x, y, z)"""
    out = np.zeros((6, S, S, S), np.int64)
    for x, y, z, d, nr, ns in unpack(records).tolist():
        a = d >> 1
        e = [1, 1, 1]
        e[RUN[a]], e[STACK[a]] = nr, ns
        out[d, x:x + e[0], y:y + e[1], z:z + e[2]] += 1
    return out
