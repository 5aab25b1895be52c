"""The yardstick of the contact tests (include/vrc.h: vrc_rigid_contacts), numpy and Python integers only.  ids are uint32
[x, y, z] arrays with NONE outside the pieces (components_model.label), worlds dense uint8 [x, y, z] arrays of 0 / 1, maps
(m, t) pairs as in rigid_model.  A record is the tuple (posed, overlap, [overlap_s1 x3], [overlap_n x3], touch, [touch_s1 x3],
[touch_n x3]) of Python integers.  The posed set of a piece is stamp_model.stamp's, exactly what rigid_model.place_affine
writes for that piece alone (tests/test_volume_contacts_host.py holds the two against each other); everything after it is
brute force over the voxels of the set.  The case generators of the GPU tests live here so that the host test can check them."""
from fractions import Fraction
from math import isqrt

import numpy as np

import components_model
import rigid_model
import stamp_model

NONE = components_model.NO_COMPONENT
ZERO = (0, 0, [0, 0, 0], [0, 0, 0], 0, [0, 0, 0], [0, 0, 0])
AXES = np.eye(3, dtype=np.int64)


def posed(ids, i, mp, box, Sd):
    """A_i as a dense uint8 array of Sd^3: piece i alone placed into zeros through mp = (m, t) inside box (lo + hi; None: all)"""
    zeros = np.zeros((Sd, Sd, Sd), np.uint8)
    if not rigid_model.map_legal(*mp):
        return zeros
    box = (0, 0, 0, Sd, Sd, Sd) if box is None else [int(v) for v in box]
    return stamp_model.stamp(zeros, (ids == i).astype(np.uint8), mp[0], mp[1], box[:3], box[3:], stamp_model.OR)


def walled(world):
    """W* of a world: the dense array inside a shell of ones -- the faces are walls; voxel p is at p + 1"""
    S = world.shape[0]
    star = np.ones((S + 2, S + 2, S + 2), np.uint8)
    star[1:-1, 1:-1, 1:-1] = np.asarray(world) != 0
    return star


def record(A, star):
    """the contact record of the posed set A (dense, or None for a skipped piece) against the world whose W* is `star`"""
    return record_at(np.argwhere(A) if A is not None else (), star)


def record_at(p, star):
    """the same from the voxels of the posed set as an (N, 3) list: what the large cases keep in place of a dense array a piece"""
    p = np.asarray(p, np.int64).reshape(-1, 3)
    if not len(p):
        return ZERO
    c = 2 * p + 1
    lower = np.stack([star[tuple((p + 1 - AXES[a]).T)] for a in range(3)], 1).astype(np.int64)
    upper = np.stack([star[tuple((p + 1 + AXES[a]).T)] for a in range(3)], 1).astype(np.int64)
    normal = lower - upper
    inside = star[tuple((p + 1).T)] != 0
    touch = ~inside & ((lower + upper).sum(1) > 0)

    def sums(sel):
        return int(sel.sum()), [int(v) for v in c[sel].sum(0)], [int(v) for v in normal[sel].sum(0)]
    return (len(p),) + sums(inside) + sums(touch)


def posed_sets(ids, maps, boxes, Sd, keep=None):
    """A_i per map (None for a piece with keep[i] == 0): what several worlds of one size share"""
    return [None if keep is not None and not keep[i] else posed(ids, i, mp, None if boxes is None else boxes[i], Sd) for i, mp in enumerate(maps)]


def contacts(ids, maps, boxes, world, keep=None):
    """one record per map: piece i posed by maps[i] inside boxes[i] (None: all of world) against world"""
    star = walled(world)
    return [record(A, star) for A in posed_sets(ids, maps, boxes, world.shape[0], keep)]


def record_tuple(rec):
    """a capi.CONTACT_DTYPE record in the model's form; its reserved word must be 0"""
    assert int(rec["reserved"]) == 0
    return (int(rec["posed"]), int(rec["overlap"]), [int(v) for v in rec["overlap_s1"]], [int(v) for v in rec["overlap_n"]],
            int(rec["touch"]), [int(v) for v in rec["touch_s1"]], [int(v) for v in rec["touch_n"]])


def contact_properties(rec, bits=200):
    """(overlap_centre, overlap_normal, touch_centre, touch_normal), three Fractions each: the centroids s1 / (2 count) exactly,
    the unit normals n / |n| with |n| from the integer root of |n|^2 4^bits, so within 2^-bits of the irrational value; zeros
    where the count or the vector is zero"""
    out = []
    for count, s1, n in ((rec[1], rec[2], rec[3]), (rec[4], rec[5], rec[6])):
        out.append([Fraction(v, 2 * count) for v in s1] if count else [Fraction(0)] * 3)
        nn = sum(v * v for v in n)
        out.append([Fraction(v << bits, isqrt(nn << (2 * bits))) for v in n] if nn else [Fraction(0)] * 3)
    return tuple(out)


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------

def worlds(S, seed):
    """the three worlds of the random test: half of the voxels at random, 2 % at random, and a half-space with a rough top"""
    rng = np.random.default_rng(seed)
    dense = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    sparse = (rng.random((S, S, S)) < 0.02).astype(np.uint8)
    height = S // 2 + rng.integers(-2, 3, (S, S))
    ground = (np.arange(S)[None, :, None] < height[:, None, :]).astype(np.uint8)          # solid below a height in y that varies with x, z
    return [("dense", dense), ("sparse", sparse), ("ground", ground)]


def specks(S=32):
    """64 isolated one-voxel pieces on a pitch of 4 in x and y at z = 5: (the dense volume, ids, records); piece i = 8 ix + iy
    sits at (4 ix + 1, 4 iy + 1, 5)"""
    vol = np.zeros((S, S, S), np.uint8)
    vol[1::4, 1::4, 5] = 1
    ids, rec = components_model.label(vol, 6)
    assert len(rec) == (S // 4) ** 2 and (rec["voxels"] == 1).all()
    return vol, ids, rec


DIRECTIONS = [(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]           # (axis, sign) of the obstacle as seen from the piece


def bit_position_case(axis, sign, S=32):
    """Every bit position of an occupancy word with an obstacle on one side.  Piece i < 32 of specks() is moved to the voxel
    with bit index i of its word (x & 1 = i & 1, y & 1 = i >> 1 & 1, z & 7 = i >> 2) in a column of 4 x 4 of its own, in the
    second word of the row (z = 8 .. 15), with a one-voxel obstacle at p + sign e_axis; piece 32 + i is moved the same way in
    another column and the world is also solid AT its voxel.  x and y take the values 2 (even) and 1 (odd) of the column, so
    the obstacle of a -x / +x neighbour lies in the next brick row for half of the positions, and for z = 8 / 15 in the word
    before / after.  Returns (ids, targets (64, 3), maps, boxes, world, expected records written out by hand)."""
    _, ids, rec = specks(S)
    world = np.zeros((S, S, S), np.uint8)
    targets, expected = np.zeros((64, 3), np.int64), []
    e = AXES[axis] * sign
    for piece in range(64):
        i, column = piece % 32, piece
        p = np.array([4 * (column // 8) + (1 if i & 1 else 2), 4 * (column % 8) + (1 if i & 2 else 2), 8 + (i >> 2)])
        assert (p[0] & 1, p[1] & 1, p[2] & 7) == (i & 1, (i >> 1) & 1, i >> 2)
        targets[piece] = p
        world[tuple(p + e)] = 1
        c, n = [int(2 * v + 1) for v in p], [int(-v) for v in e]           # the normal points from the obstacle to the piece
        if piece < 32:
            expected.append((1, 0, [0, 0, 0], [0, 0, 0], 1, c, n))
        else:
            world[tuple(p)] = 1
            expected.append((1, 1, c, n, 0, [0, 0, 0], [0, 0, 0]))
    offsets = targets - rec["lo"].astype(np.int64)
    return ids, targets, rigid_model.translation_maps(offsets), rigid_model.moved_boxes(rec, offsets, S), world, expected


def wall_case(S=32):
    """eight 3 x 3 x 3 blocks, posed against an empty world: piece k < 6 flat against face k (a VRC_FACE_* code: -x, +x, -y,
    +y, -z, +z), piece 6 in the corner (0, 0, 0), piece 7 with one of its layers beyond the face x = S.  Returns (the blocks'
    volume, offsets (8, 3)); the blocks are alike, so which one goes where does not matter."""
    vol = np.zeros((S, S, S), np.uint8)
    for k in range(8):
        vol[4 + 6 * (k % 4):7 + 6 * (k % 4), 4 + 6 * (k // 4):7 + 6 * (k // 4), 10:13] = 1
    _, rec = components_model.label(vol, 6)
    at = [(0, 14, 18), (S - 3, 14, 18), (10, 0, 18), (10, S - 3, 18), (10, 14, 0), (10, 14, S - 3), (0, 0, 0), (S - 2, 14, 18)]
    return vol, np.array(at, np.int64) - rec["lo"].astype(np.int64)


def end_to_end_case(S=32):
    """a floor with a pillar, a sphere dug through the pillar, and a loose block in the air: (the volume, its supported part,
    the debris), the scene of the rigid tests' end-to-end case; down is -y"""
    vol = np.zeros((S, S, S), np.uint8)
    vol[:, 0:3, :] = 1
    vol[14:18, 3:28, 14:18] = 1
    x, y, z = np.indices((S, S, S))
    vol[(x - 16) ** 2 + (y - 12) ** 2 + (z - 16) ** 2 <= 25] = 0
    vol[4:9, 20:23, 5:12] = 1
    whole, _ = components_model.label(vol, 6)
    supported = (whole == whole[0, 0, 0]).astype(np.uint8)
    return vol, supported, vol & (1 - supported)
