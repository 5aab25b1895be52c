"""The yardstick of the rigid-piece tests (include/vrc.h: vrc_rigid_moments, vrc_rigid_place_affine, vrc_affine_place_box),
numpy and Python integers only.  ids are uint32 [x, y, z] arrays with NONE outside the pieces (components_model.label),
volumes dense uint8 [x, y, z] arrays of 0 / 1.  The map arithmetic is stamp_model's, the case generators of the GPU tests live
here so that the host test can check them."""
from fractions import Fraction

import numpy as np

import components_model
import stamp_model

NONE = components_model.NO_COMPONENT
OR, ANDNOT = stamp_model.OR, stamp_model.ANDNOT
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def moments(ids, C=None):
    """[(n, [s1 x3], [s2 x6])] per piece, by brute force in Python integers: c = 2p + 1"""
    inside = ids != NONE
    xyz = np.argwhere(inside)
    pid = ids[inside].astype(np.int64)
    if C is None:
        C = int(pid.max()) + 1 if len(pid) else 0
    out = [[0, [0, 0, 0], [0, 0, 0, 0, 0, 0]] for _ in range(C)]
    for p, i in zip(xyz.tolist(), pid.tolist()):
        c = [2 * v + 1 for v in p]
        rec = out[i]
        rec[0] += 1
        for a in range(3):
            rec[1][a] += c[a]
        for j, (a, b) in enumerate(PAIRS):
            rec[2][j] += c[a] * c[b]
    return [(n, s1, s2) for n, s1, s2 in out]


def moments_fast(ids, C):
    """the same by numpy in int64 (exact: every sum is below 2^53), for volumes too large for the loop"""
    inside = ids != NONE
    c = 2 * np.argwhere(inside).astype(np.int64) + 1
    pid = ids[inside].astype(np.int64)
    cols = [np.ones(len(pid), np.int64)] + [c[:, a] for a in range(3)] + [c[:, a] * c[:, b] for a, b in PAIRS]
    sums = np.zeros((C, 10), np.int64)
    for k, col in enumerate(cols):
        np.add.at(sums[:, k], pid, col)
    return [(row[0], row[1:4], row[4:10]) for row in sums.tolist()]


def moments_tuple(rec):
    """a capi.MOMENTS_DTYPE record in the model's form"""
    return int(rec["voxels"]), [int(v) for v in rec["s1"]], [int(v) for v in rec["s2"]]


def solid_cube_moments(S):
    """a full S^3 cube in closed form: sum of c = S^2 and of c^2 = S (4 S^2 - 1) / 3 over c = 1, 3, .. 2S-1"""
    n, one, two = S ** 3, S * S, S * (4 * S * S - 1) // 3
    return n, [one * S * S] * 3, [two * S * S] * 3 + [one * one * S] * 3


def mass_properties(n, s1, s2):
    """(mass, centre, inertia) as exact Fractions: a voxel is a unit cube of unit mass"""
    central = {ab: Fraction(s2[j], 4) - Fraction(s1[ab[0]] * s1[ab[1]], 4 * n) for j, ab in enumerate(PAIRS)}
    centre = [Fraction(s1[a], 2 * n) for a in range(3)]
    inertia = [[None] * 3 for _ in range(3)]
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        inertia[a][a] = central[(b, b)] + central[(c, c)] + Fraction(n, 6)
    for a, b in PAIRS[3:]:
        inertia[a][b] = inertia[b][a] = -central[(a, b)]
    return Fraction(n), centre, inertia


def map_legal(m, t, reserved=0):
    return reserved == 0 and max(abs(int(v)) for v in m) <= stamp_model.M_LIMIT and max(abs(int(v)) for v in t) <= stamp_model.T_LIMIT


def place_affine(ids, maps, boxes, base, op=OR, keep=None):
    """a copy of `base` (any size) with every kept piece i gathered through maps[i] = (m, t) inside boxes[i] (lo + hi, 6
    numbers; boxes None: all of base): the source of piece i is the volume { ids == i }.  A map beyond the limits drops its piece."""
    out = (np.asarray(base) != 0).astype(np.uint8)
    Sd = out.shape[0]
    for i, (m, t) in enumerate(maps):
        if keep is not None and not keep[i]:
            continue
        if not map_legal(m, t):
            continue
        box = (0, 0, 0, Sd, Sd, Sd) if boxes is None else [int(v) for v in boxes[i]]
        out = stamp_model.stamp(out, (ids == i).astype(np.uint8), m, t, box[:3], box[3:], op)
    return out


def translation_maps(offsets):
    """the inverse maps of "piece i moves by offsets[i]": q = p - offset"""
    return [(list(stamp_model.IDENTITY[0]), [-int(o) << 17 for o in off]) for off in np.asarray(offsets).reshape(-1, 3)]


def moved_boxes(records, offsets, S):
    """the record boxes moved by the offsets and clipped to [0, S], as (C, 6) uint32; a box that leaves the volume becomes empty"""
    out = np.zeros((len(records), 6), np.uint32)
    for i, off in enumerate(np.asarray(offsets, np.int64).reshape(-1, 3)):
        lo = np.clip(records["lo"][i].astype(np.int64) + off, 0, S)
        hi = np.clip(records["hi"][i].astype(np.int64) + off, 0, S)
        out[i] = list(lo) + list(hi)
    return out


def place_box(rot, scale, src_pivot, dst_pivot, src_lo, src_hi, dst_depth):
    """vrc_affine_place_box restated in Python doubles: stamp_model.place's map, the box from the corners of [src_lo, src_hi]"""
    m, t, _, _ = stamp_model.place(rot, scale, src_pivot, dst_pivot, 2, dst_depth)
    rot = [float(np.float32(v)) for v in np.asarray(rot).reshape(9)]
    scale = float(np.float32(scale))
    sp = [float(np.float32(v)) for v in src_pivot]
    dp = [float(np.float32(v)) for v in dst_pivot]
    ends = [(float(int(src_lo[c])), float(int(src_hi[c]))) for c in range(3)]
    Sd = float(1 << dst_depth)
    lo, hi = [0] * 3, [0] * 3
    for r in range(3):
        xs = []
        for corner in range(8):
            x = dp[r]
            for c in range(3):
                x += scale * rot[3 * c + r] * (ends[c][(corner >> c) & 1] - sp[c])
            xs.append(x)
        lo[r] = int(max(np.floor(min(xs)) - 2.0, 0.0))
        hi[r] = int(min(np.ceil(max(xs)) + 2.0, Sd))
    if any(l >= h for l, h in zip(lo, hi)):
        lo, hi = [0] * 3, [0] * 3
    return m, t, lo, hi


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------

def random_debris(S, seed):
    """boxes and specks in the air: pieces of many sizes, some touching by an edge or a corner (separate under 6-connectivity)"""
    rng = np.random.default_rng(seed)
    vol = np.zeros((S, S, S), np.uint8)
    for _ in range(S):
        lo = rng.integers(0, S, 3)
        size = rng.integers(1, max(2, S // 4), 3)
        vol[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = 1
    vol[rng.random((S, S, S)) < 0.02] = 1
    return vol


def combs(S):
    """two interlocking combs: piece A is the plane x = 0 with teeth at z = 0 mod 4 that reach x = S-3, piece B the plane
    x = S-1 with teeth at z = 2 mod 4 that reach back to x = 2; the odd z layers between the teeth are empty.  For
    2 <= x < S-2 every occupancy word (2 x 2 x 8 voxels, 8 along z) holds voxels of exactly the two pieces, two z layers each,
    so a wave of 64 keys there has two ids."""
    vol = np.zeros((S, S, S), np.uint8)
    vol[0, :, :] = 1
    vol[S - 1, :, :] = 1
    vol[0:S - 2, :, 0::4] = 1
    vol[2:S, :, 2::4] = 1
    return vol


def checkerboard(S):
    x, y, z = np.indices((S, S, S))
    return ((x + y + z) & 1).astype(np.uint8)


def pose_case(S, seed):
    """(debris, maps, boxes, keep, base) for the many-piece placement test: touching blocks on a grid, so that a turned box
    of one piece covers voxels of its neighbours; the maps are seeded signed permutations about the piece's own box centre for
    the even pieces and general rotations about it for the odd ones, a few aimed at one common spot so that pieces overlap;
    the boxes are generous, with odd corners, and some are clipped, empty or inverted; one map reads far outside the source."""
    rng = np.random.default_rng(seed)
    debris = np.zeros((S, S, S), np.uint8)
    # blocks of 5 x 4 x 6 on a pitch of 6 x 5 x 7, joined to their x neighbours by nothing: they touch diagonally through a
    # corner voxel added to each, which 6-connectivity keeps apart
    for bx in range(1, S - 6, 6):
        for by in range(1, S - 5, 5):
            for bz in range(1, S - 7, 7):
                debris[bx:bx + 5, by:by + 4, bz:bz + 6] = 1
                debris[bx + 5, by + 4, bz + 6] = 1 if rng.random() < 0.5 else 0       # a speck of its own touching two blocks by corners
                if rng.random() < 0.3:
                    debris[bx + 1:bx + 3, by + 1:by + 3, bz:bz + 6] = 0                # a hole through it
    debris[:, :, S - 1] = 0
    ids, rec = components_model.label(debris, 6)
    C = len(rec)
    perms = stamp_model.all_signed_permutations()
    maps, boxes = [], np.zeros((C, 6), np.uint32)
    spot = np.array([S // 2, S // 2, S // 2], np.float64)
    for i in range(C):
        lo, hi = rec["lo"][i].astype(np.float64), rec["hi"][i].astype(np.float64)
        centre = (lo + hi) / 2
        target = spot if i % 7 == 3 else centre + rng.integers(-3, 4, 3)
        if i % 2 == 0:
            perm, flip = perms[int(rng.integers(len(perms)))]
            m = [0] * 9
            for a in range(3):
                m[3 * a + perm[a]] = -stamp_model.ONE if flip[a] else stamp_model.ONE
            # q - centre = m (p - target): t in units of 2^-17, the centres doubled are integers
            t = [int(2 * centre[a]) * 65536 - sum(m[3 * a + b] * int(2 * target[b]) for b in range(3)) for a in range(3)]
        else:
            rot = stamp_model.compose(stamp_model.rotation(0, rng.uniform(0, 6.28)), stamp_model.rotation(int(rng.integers(1, 3)), rng.uniform(0, 6.28)))
            m, t, _, _ = stamp_model.place(rot, float(rng.choice([1.0, 1.0, 0.75, 1.5])), centre, target, 5, 5)
        reach = int(np.ceil(np.linalg.norm(hi - lo))) + 2
        blo = np.clip(np.floor(target) - reach + rng.integers(0, 2, 3), 0, S).astype(np.int64)
        bhi = (np.floor(target) + reach + rng.integers(0, 2, 3)).astype(np.int64)     # may lie beyond S: clipped by the call
        boxes[i] = list(blo) + list(bhi)
        maps.append((m, t))
    if C > 12:
        boxes[5] = [4, 4, 4, 4, 9, 9]                   # empty
        boxes[6] = [9, 3, 3, 5, 8, 8]                   # inverted
        boxes[8, 3:] = 0xFFFFFFFF                       # clipped to dst
        maps[9] = (maps[9][0], [v + (300 << 17) for v in maps[9][1]])                 # reads 300 voxels outside the source
        boxes[10] = [0, 0, 0, S, S, S]
    keep = (rng.random(C) < 0.8).astype(np.uint8)
    base = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    return debris, ids, maps, boxes, keep, base
