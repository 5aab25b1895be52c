"""The yardstick of the pair-contact tests (include/vrc.h: vrc_rigid_pair_contacts, vrc_rigid_box_pairs), numpy and Python
integers only, built from contact_model: the posed sets are contact_model.posed_sets', the record is contact_model.record's,
and the world of pair (a, b) is A_b inside a shell of ZEROS -- between pieces there are no walls.  box_pairs is the brute-force
double loop over the clipped boxes.  The case generators of the GPU tests live here so that the host test can check them."""
import numpy as np

import components_model
import contact_model
import rigid_model

NONE = components_model.NO_COMPONENT
ZERO = contact_model.ZERO


def unwalled(A):
    """W* of the world A_b: the dense set inside a shell of zeros; voxel p is at p + 1"""
    S = A.shape[0]
    star = np.zeros((S + 2, S + 2, S + 2), np.uint8)
    star[1:-1, 1:-1, 1:-1] = np.asarray(A) != 0
    return star


def records_of(sets, pairs, Sd):
    """one record per pair from the posed sets (None: a piece with keep == 0); an index beyond the pieces gives ZERO"""
    empty = np.zeros((Sd, Sd, Sd), np.uint8)
    stars = {}
    out = []
    for a, b in np.asarray(pairs, np.int64).reshape(-1, 2):
        if a >= len(sets) or b >= len(sets):
            out.append(ZERO)
            continue
        if b not in stars:
            stars[b] = unwalled(empty if sets[b] is None else sets[b])
        out.append(contact_model.record(sets[a], stars[b]))
    return out


def pair_contacts(ids, maps, boxes, pairs, Sd, keep=None):
    """one record per ordered pair (a, b): piece a posed by maps[a] inside boxes[a] (None: all of the posed volume of Sd^3)
    against piece b posed the same way and nothing else"""
    return records_of(contact_model.posed_sets(ids, maps, boxes, Sd, keep), pairs, Sd)


def clipped(box, Sd):
    """(lo, hi) of a box clipped to [0, Sd)^3, or None where it is empty or inverted"""
    lo, hi = [int(v) for v in box[:3]], [min(int(v), Sd) for v in box[3:]]
    return (lo, hi) if all(l < h for l, h in zip(lo, hi)) else None


def box_pairs(boxes, Sd, keep=None):
    """the candidate pairs as an (P, 2) uint32 array, (a, b) ascending: a != b, both kept with a box, and on every axis
    lo_a <= hi_b and lo_b <= hi_a (hi exclusive)"""
    live = [clipped(box, Sd) if keep is None or keep[i] else None for i, box in enumerate(np.asarray(boxes).reshape(-1, 6))]
    out = []
    for a, A in enumerate(live):
        for b, B in enumerate(live):
            if a != b and A and B and all(A[0][x] <= B[1][x] and B[0][x] <= A[1][x] for x in range(3)):
                out.append((a, b))
    return np.array(out, np.uint32).reshape(-1, 2)


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------

def bit_position_case(axis, sign, overlap, S=32):
    """Every bit position of an occupancy word with a one-voxel piece b on one side.  contact_model.specks gives 64 one-voxel
    pieces; piece i < 32 (a) is moved to the voxel with bit index i of its word, in a column of 4 x 4 of its own, in the
    second word of the row (z = 8 .. 15), exactly as contact_model.bit_position_case places it, and piece 32 + i (b) to
    p + sign e_axis -- or, with overlap, onto p itself.  Returns (ids, maps, boxes, pairs (32, 2), expected records written
    out by hand)."""
    _, ids, rec = contact_model.specks(S)
    e = contact_model.AXES[axis] * sign
    targets, pairs, expected = np.zeros((64, 3), np.int64), [], []
    for i in range(32):
        p = np.array([4 * (i // 8) + (1 if i & 1 else 2), 4 * (i % 8) + (1 if i & 2 else 2), 8 + (i >> 2)])
        assert (p[0] & 1, p[1] & 1, p[2] & 7) == (i & 1, (i >> 1) & 1, i >> 2)
        targets[i], targets[32 + i] = p, p if overlap else p + e
        pairs.append((i, 32 + i))
        c, n = [int(2 * v + 1) for v in p], [int(-v) for v in e]               # the normal points out of b towards a
        expected.append((1, 1, c, [0, 0, 0], 0, [0, 0, 0], [0, 0, 0]) if overlap else (1, 0, [0, 0, 0], [0, 0, 0], 1, c, n))
    offsets = targets - rec["lo"].astype(np.int64)
    return ids, rigid_model.translation_maps(offsets), rigid_model.moved_boxes(rec, offsets, S), np.array(pairs, np.uint32), expected


def inner_blocks(S=32, seed=3):
    """blocks in the air of an S^3 volume and offsets that keep every moved block at least one voxel away from the faces, some
    onto each other: (the volume, offsets (C, 3)); the case in which the no-walls rule and the walled one agree"""
    rng = np.random.default_rng(seed)
    vol = np.zeros((S, S, S), np.uint8)
    for k in range(6):
        x, y = 3 + 9 * (k % 3), 3 + 12 * (k // 3)
        vol[x:x + 2 + k % 3, y:y + 3, 5:9 + k] = 1
    _, rec = components_model.label(vol, 6)
    spot = np.array([12, 12, 12])
    offsets = np.array([spot + rng.integers(-2, 3, 3) - r["lo"].astype(np.int64) for r in rec])
    for r, off in zip(rec, offsets):
        assert ((r["lo"].astype(np.int64) + off) >= 1).all() and ((r["hi"].astype(np.int64) + off) <= S - 1).all()
    return vol, offsets


def turned_case(vol, connectivity, Sd, seed):
    """(ids, rec, maps, boxes, keep) for a labelling of `vol` posed into Sd^3: every piece under a small turn of its own about
    its box centre, the pieces drawn towards the middle so that they meet and overlap, with boxes generous by two voxels, and
    a keep mask that leaves about 120 pieces, so that the candidate pairs stay a few thousand.  Maps as (m, t)."""
    import stamp_model
    rng = np.random.default_rng(seed)
    ids, rec = components_model.label(vol, connectivity)
    S = vol.shape[0]
    maps, boxes = [], np.zeros((len(rec), 6), np.uint32)
    for i, r in enumerate(rec):
        lo, hi = r["lo"].astype(np.float64), r["hi"].astype(np.float64)
        centre = (lo + hi) / 2
        target = Sd / 2 + (centre - S / 2) * (0.55 * Sd / 32) + rng.uniform(-1, 1, 3)
        ax, ay = rng.uniform(-0.5, 0.5, 2)
        cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
        R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        inv = R.T                                                               # q - centre = R^T (p - target)
        m = [int(round(v * stamp_model.ONE)) for v in inv.reshape(9)]
        # s = m (2p + 1) + t with q = s >> 17 and ONE = 2^16 per half voxel: t = 2^17 (centre - inv target)
        t = [int(round(v * (1 << 17))) for v in centre - inv @ target]
        maps.append((m, t))
        half = np.abs(R) @ ((hi - lo) / 2) + 2
        boxes[i, :3] = np.clip(np.floor(target - half), 0, Sd)
        boxes[i, 3:] = np.clip(np.ceil(target + half), 0, Sd)
    keep = (rng.random(len(rec)) < 120 / max(len(rec), 120)).astype(np.uint8)
    return ids, rec, maps, boxes, keep
