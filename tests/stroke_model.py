"""The capsule brush restated in numpy (include/vrc.h: vrc_stroke_fill_capsules, vrc_stroke_fill_at_hits): the rule in int64
over a capsule's clipped bounding box, the same rule slab by slab for volumes too large for that, the dropped-item rules, and
the items of a stroke through centres; beside them the scan line of rays that the hit tests share.  Nothing here is taken from csrc/vrc_stroke.h: no piece size, no box arithmetic."""
import ctypes as C

import numpy as np

LIMIT = 8192


def kept(item):
    """the item is not dropped: coordinates and radius within the limit, reserved 0 (r < 0 is kept, and empty)"""
    item = [int(v) for v in item]
    return all(abs(c) <= LIMIT for c in item[:6]) and item[6] <= LIMIT and item[7] == 0


def rule(x, y, z, item):
    """the membership rule on int64 arrays x, y, z (broadcast against one another)"""
    ax, ay, az, bx, by, bz, r = [int(v) for v in item[:7]]
    dx, dy, dz = bx - ax, by - ay, bz - az
    L2 = dx * dx + dy * dy + dz * dz
    qx, qy, qz = x - ax, y - ay, z - az
    qq = qx * qx + qy * qy + qz * qz
    t = qx * dx + qy * dy + qz * dz
    pb = (x - bx) ** 2 + (y - by) ** 2 + (z - bz) ** 2
    at_a = (t <= 0) | (L2 == 0)
    at_b = ~at_a & (t >= L2)
    return np.where(at_a, qq <= r * r, np.where(at_b, pb <= r * r, qq * L2 - t * t <= r * r * L2))


def rule_int(p, item):
    """the rule for one voxel in Python integers: no width at all"""
    ax, ay, az, bx, by, bz, r = [int(v) for v in item[:7]]
    d = (bx - ax, by - ay, bz - az)
    q = (int(p[0]) - ax, int(p[1]) - ay, int(p[2]) - az)
    L2 = sum(v * v for v in d)
    qq = sum(v * v for v in q)
    t = sum(u * v for u, v in zip(q, d))
    if r < 0:
        return False
    if L2 == 0 or t <= 0:
        return qq <= r * r
    if t >= L2:
        return sum((int(p[i]) - (bx, by, bz)[i]) ** 2 for i in range(3)) <= r * r
    return qq * L2 - t * t <= r * r * L2


def bounding_box(S, item):
    """the capsule's bounding box clipped to the volume, (lo, hi) with hi exclusive, or None"""
    a, b, r = np.array(item[0:3], np.int64), np.array(item[3:6], np.int64), int(item[6])
    if r < 0:
        return None
    lo = np.maximum(np.minimum(a, b) - r, 0)
    hi = np.minimum(np.maximum(a, b) + r + 1, S)
    return None if (lo >= hi).any() else (lo, hi)


def capsule_voxels(S, item):
    """(k, 3) int64: the voxels of the item inside S^3, over its clipped bounding box"""
    box = bounding_box(S, item) if kept(item) else None
    if box is None:
        return np.zeros((0, 3), np.int64)
    lo, hi = box
    x, y, z = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    return np.argwhere(rule(x.astype(np.int64), y.astype(np.int64), z.astype(np.int64), item)) + lo


def capsule_voxels_sparse(S, item, slab=8, pad=3.0):
    """the same for thin capsules in large volumes: slabs of the major axis, each with the float bounding box of the stretch
    of the segment that can reach it, padded by `pad` voxels beyond the radius; every voxel of the box is put to the exact rule"""
    box = bounding_box(S, item) if kept(item) else None
    if box is None:
        return np.zeros((0, 3), np.int64)
    a, b, r = np.array(item[0:3], np.float64), np.array(item[3:6], np.float64), int(item[6])
    d = b - a
    M = int(np.argmax(np.abs(d)))
    out = []
    for m0 in range(int(box[0][M]), int(box[1][M]), slab):
        m1 = min(m0 + slab, int(box[1][M]))
        if d[M] == 0:
            ends = np.stack([a, a])
        else:
            u = np.clip((np.array([m0 - r - pad, m1 + r + pad]) - a[M]) / d[M], 0.0, 1.0)
            ends = a[None, :] + u[:, None] * d[None, :]
        lo = np.maximum(np.floor(ends.min(axis=0) - r - pad).astype(np.int64), 0)
        hi = np.minimum(np.ceil(ends.max(axis=0) + r + pad).astype(np.int64) + 1, S)
        lo[M], hi[M] = m0, m1
        if (lo >= hi).any():
            continue
        x, y, z = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        out.append(np.argwhere(rule(x.astype(np.int64), y.astype(np.int64), z.astype(np.int64), item)) + lo)
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def fill_capsules(dense, items, value, sparse=False):
    """dense[x, y, z] = value at every voxel of every item, in place"""
    S = dense.shape[0]
    for item in np.asarray(items, np.int64).reshape(-1, 8).tolist():
        p = capsule_voxels_sparse(S, item) if sparse else capsule_voxels(S, item)
        dense[p[:, 0], p[:, 1], p[:, 2]] = value
    return dense


def stroke_items(centres, valid, radius, max_gap):
    """(k, 8) int32: item i of vrc_stroke_fill_at_hits for every record that gives one -- the capsule to the next centre where
    both are valid and the step is within max_gap (0: any step), else the ball at the centre"""
    centres = np.asarray(centres, np.int64).reshape(-1, 3)
    out = []
    for i in range(len(centres)):
        if not valid[i]:
            continue
        b = centres[i]
        if i + 1 < len(centres) and valid[i + 1]:
            step = centres[i + 1] - centres[i]
            if max_gap == 0 or int((step * step).sum()) <= max_gap * max_gap:
                b = centres[i + 1]
        out.append(list(centres[i]) + list(b) + [radius, 0])
    return np.array(out, np.int64).reshape(-1, 8).astype(np.int32)


def mixed_items(rng, S, count):
    """axis-aligned, diagonal and degenerate capsules with r in {0, 1, 2, 5} and -1, ends far outside the volume, items over the
    limit and items with reserved != 0"""
    a = rng.integers(-4, S + 4, (count, 3))
    b = rng.integers(-4, S + 4, (count, 3))
    kind = rng.integers(0, 8, count)
    b[kind == 0] = a[kind == 0]                                               # degenerate
    for i in np.flatnonzero(kind == 1):                                        # axis-aligned
        keep = rng.integers(0, 3)
        b[i] = a[i]
        b[i, keep] = rng.integers(-4, S + 4)
    for i in np.flatnonzero(kind == 2):                                        # an exact diagonal: ties of the major axis
        b[i] = a[i] + rng.integers(1, S) * rng.choice([-1, 1], 3)
    far = np.flatnonzero(kind == 3)                                            # ends far outside
    a[far, rng.integers(0, 3, len(far))] = -rng.integers(S, LIMIT + 1, len(far))
    b[far, rng.integers(0, 3, len(far))] = rng.integers(S, LIMIT + 1, len(far))
    r = rng.choice([0, 1, 2, 5, 0, 1, 2, 5, -1], (count, 1))
    items = np.concatenate([a, b, r, np.zeros((count, 1), np.int64)], axis=1)
    over = np.flatnonzero(kind == 4)
    items[over[0::3], 0] = LIMIT + 1                                           # dropped: a coordinate, the radius, reserved
    items[over[1::3], 6] = LIMIT + 1
    items[over[2::3], 7] = rng.choice([1, -1, 1 << 30], len(over[2::3]))
    return items.astype(np.int32)


def triangle(v, lo, hi):
    """v folded into [lo, hi]: a path that turns round at the walls keeps its step length"""
    span = hi - lo
    w = np.mod(v - lo, 2 * span)
    return lo + np.where(w > span, 2 * span - w, w)


def scan_rays(depth, n, step, varied=True, start=(5.3, 9.7), heading=(0.8, 0.6)):
    """A crosshair dragged over the terrain: n nearly parallel rays from outside the volume on the open side of the terrain
    (small y in the walk's space), their origins `step` voxels apart on average along a slanted path -- with varied, between 0 and
    2.4 `step` -- so successive hits lie that far apart plus the terrain's relief; every 13th ray points away (a miss)"""
    f = np.float32
    S = float(1 << depth)
    w = np.tile([0.0, 0.3, 1.0, 2.4, 0.7, 1.6], n // 6 + 1)[:n] if varied else np.ones(n)
    s = np.cumsum(w * step)
    x = triangle(start[0] + heading[0] * s, 3.0, S - 3.0)
    z = triangle(start[1] + heading[1] * s, 3.0, S - 3.0)
    org = np.stack([1.0 + x / S, np.full(n, 0.9), 1.0 + z / S], -1).astype(f)
    d = np.tile(np.array([0.05, 1.0, 0.03]) / np.linalg.norm([0.05, 1.0, 0.03]), (n, 1))
    d[12::13] *= -1.0
    return org, d.astype(f)


def gaps_of(centres, valid):
    """the lengths of the steps between successive valid centres"""
    return np.array([np.sqrt(float(((centres[i + 1] - centres[i]) ** 2).sum())) for i in range(len(centres) - 1) if valid[i] and valid[i + 1]])


def hit_centres(depth, records, solid):
    """(centres (n, 3) int64, valid (n,) bool): the library's host function vrc_hit_to_voxel per record, as the brush tests use
    it -- dig at the voxel, build at the neighbour; a refused record, and a build without a neighbour, is not valid"""
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    records = np.ascontiguousarray(records, vrc.HIT_DTYPE)
    voxel, neighbour, has = np.zeros(3, np.uint32), np.zeros(3, np.uint32), C.c_int()
    pv, pn, ph = vrc.capi.ptr(voxel), vrc.capi.ptr(neighbour), C.byref(has)
    centres, valid = np.zeros((len(records), 3), np.int64), np.zeros(len(records), bool)
    for i in range(len(records)):
        if L.vrc_hit_to_voxel(depth, C.c_void_p(records.ctypes.data + 48 * i), pv, pn, ph) != 0:
            continue
        if solid and not has.value:
            continue
        centres[i], valid[i] = (neighbour if solid else voxel), True
    return centres, valid
