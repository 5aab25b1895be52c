"""The yardstick of the fall tests (include/vrc.h: vrc_fall_drops, vrc_fall_place), numpy only.

The drops come from the literal TICK SIMULATION, not from the constraint system the device relaxes: at every tick the
largest set of pieces that can all move one cell together moves.  A piece is blocked if it overlaps F, if a voxel of it has
F or the wall in the next cell, if it has fallen drop_limit cells, or if a voxel of it has a blocked piece in the next cell
(a fixed point over the "rests on" pairs).  tests/test_volume_fall_host.py holds this against the column relaxation taken
literally from the rule.  The case generators of the GPU tests live here too, so that the host test can check them."""
import numpy as np

import components_model

NONE = components_model.NO_COMPONENT
OFFSET_LIMIT = 1 << 20


def step_of(direction):
    """the unit step g of a face code 2*axis + side"""
    g = np.zeros(3, np.int64)
    g[direction >> 1] = 1 if direction & 1 else -1
    return g


def drops(ids, fixed, direction, drop_limit=0):
    """int64 D per piece: ids uint32 [x, y, z] with NONE outside the pieces, fixed uint8 [x, y, z] or None"""
    S = ids.shape[0]
    inside = ids != NONE
    xyz = np.argwhere(inside)
    pid = ids[inside].astype(np.int64)
    C = int(pid.max()) + 1 if len(pid) else 0
    F = np.zeros((S, S, S), bool) if fixed is None else np.asarray(fixed) != 0
    g = step_of(direction)
    D = np.zeros(C, np.int64)
    if C == 0:
        return D
    in_f = np.zeros(C, bool)
    in_f[pid[F[tuple(xyz.T)]]] = True
    while True:
        pos = xyz + D[pid, None] * g
        grid = np.full((S, S, S), -1, np.int64)
        grid[tuple(pos.T)] = pid
        ahead = pos + g
        wall = ((ahead < 0) | (ahead >= S)).any(axis=1)
        at = tuple(np.clip(ahead, 0, S - 1).T)
        blocked = in_f.copy()
        blocked[pid[wall | (F[at] & ~wall)]] = True
        if drop_limit:
            blocked |= D >= drop_limit
        other = np.where(wall, -1, grid[at])
        rests = (other >= 0) & (other != pid)
        pairs = np.unique(np.stack([pid[rests], other[rests]], axis=1), axis=0)      # (upper piece, the piece it rests on)
        while True:
            more = blocked.copy()
            more[pairs[blocked[pairs[:, 1]], 0]] = True
            if np.array_equal(more, blocked):
                break
            blocked = more
        if blocked.all():
            return D
        D = D + ~blocked


def offsets_of(D, direction):
    """(C, 3) int32: D_i * g"""
    return (np.asarray(D, np.int64)[:, None] * step_of(direction)).astype(np.int32).reshape(-1, 3)


def place(ids, offsets, dst, op_or=True, keep=None):
    """dst uint8 [x, y, z] with every voxel of the kept pieces, moved by its piece's offset, set (op_or) or cleared"""
    S = ids.shape[0]
    out = np.array(dst, np.uint8)
    inside = ids != NONE
    xyz = np.argwhere(inside)
    pid = ids[inside].astype(np.int64)
    offsets = np.asarray(offsets, np.int64).reshape(-1, 3)
    ok = np.ones(len(pid), bool) if keep is None else np.asarray(keep)[pid] != 0
    ok &= (np.abs(offsets) <= OFFSET_LIMIT).all(axis=1)[pid] if len(pid) else True
    target = xyz + offsets[pid] if len(pid) else xyz
    ok &= ((target >= 0) & (target < S)).all(axis=1)
    out[tuple(target[ok].T)] = 1 if op_or else 0
    return out


def stats(ids, D):
    """(moved_voxels, pieces, moved_pieces, max_drop)"""
    count = np.bincount(ids[ids != NONE].astype(np.int64), minlength=len(D))
    moved = np.asarray(D) > 0
    return int(count[moved].sum()), len(D), int(moved.sum()), int(max(D, default=0))


def stats_tuple(st):
    """the same four numbers of a capi.FallStats"""
    return int(st.moved_voxels), int(st.pieces), int(st.moved_pieces), int(st.max_drop)


def features(ids, fixed, direction, drop_limit, D):
    """what a case exercises, as a set of names: "lands_on_piece" -- a piece that moved and rests on another piece; "lower_falls_farther" --
    a piece directly ahead of another in some column that falls farther than it; "limit" -- a piece stopped by drop_limit that
    would fall farther without; "in_fixed" -- a piece with drop 0 because it overlaps F"""
    S = ids.shape[0]
    found = set()
    inside = ids != NONE
    xyz = np.argwhere(inside)
    pid = ids[inside].astype(np.int64)
    if not len(pid):
        return found
    g = step_of(direction)
    F = np.zeros((S, S, S), bool) if fixed is None else np.asarray(fixed) != 0
    if (D[np.unique(pid[F[tuple(xyz.T)]])] == 0).any():
        found.add("in_fixed")
    if drop_limit and (drops(ids, fixed, direction, 0)[D == drop_limit] > drop_limit).any():
        found.add("limit")
    # lands_on_piece: after the move, the next cell of a voxel of a piece that moved holds another piece
    where = xyz + D[pid, None] * g
    grid = np.full((S, S, S), -1, np.int64)
    grid[tuple(where.T)] = pid
    ahead = where + g
    ok = ((ahead >= 0) & (ahead < S)).all(axis=1)
    other = grid[tuple(ahead[ok].T)]
    if ((other >= 0) & (other != pid[ok]) & (D[pid[ok]] > 0)).any():
        found.add("lands_on_piece")
    # lower_falls_farther: on entry, the nearest non-empty voxel ahead of a voxel is of another piece, and that one falls farther
    grid = np.full((S, S, S), -1, np.int64)
    grid[tuple(xyz.T)] = pid
    searching = np.ones(len(pid), bool)
    for k in range(1, S):
        ahead = xyz + k * g
        searching &= ((ahead >= 0) & (ahead < S)).all(axis=1)
        at = tuple(np.clip(ahead, 0, S - 1).T)
        other = grid[at]
        hit = searching & (other >= 0)
        if (hit & (other != pid) & (D[np.maximum(other, 0)] > D[pid])).any():
            found.add("lower_falls_farther")
        searching &= ~hit & ~F[at]
    return found


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------

def random_case(S, seed):
    """(debris uint8, fixed uint8): a few dozen boxes and specks as debris in the air, a ragged floor and some ledges as F;
    every third case lets F overlap the debris"""
    rng = np.random.default_rng(seed)
    debris = np.zeros((S, S, S), np.uint8)
    fixed = np.zeros((S, S, S), np.uint8)
    for _ in range(S):
        lo = rng.integers(0, S, 3)
        size = rng.integers(1, max(2, S // 4), 3)
        debris[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = 1
    debris[rng.random((S, S, S)) < 0.01] = 1
    for _ in range(S // 2):
        lo = rng.integers(0, S, 3)
        size = rng.integers(1, max(2, S // 3), 3)
        fixed[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = 1
    if seed % 3:
        fixed[debris != 0] = 0
    return debris, fixed


RANDOM_CASES = [(S, connectivity, direction, (0, 3, 0, 1, 0, 2)[direction], 700 + 10 * direction + connectivity + S)
                for S in (16, 32) for connectivity in (6, 26) for direction in range(6)]


def plate_stack(S, direction):
    """Six plates, one voxel thick, two columns wide and as deep as the volume, as a staircase: plate k and plate k + 1 share
    one column, plate 0 is the nearest to the far face and alone stands over a block of F, and the gaps between neighbours
    are 1, 2, 3, 4 and 5 cells (S >= 24).  The chain of piece-on-piece constraints runs against the order of the columns, so a relaxation that takes
    the columns in ascending order settles one plate per round.  Returns (debris, fixed)."""
    axis, side = direction >> 1, direction & 1
    across = (axis + 1) % 3
    debris = np.zeros((S, S, S), np.uint8)
    fixed = np.zeros((S, S, S), np.uint8)
    q = 3                                               # cells between plate 0 and the far face
    for k in range(6):
        sl = [slice(None)] * 3
        sl[across] = slice(5 - k, 7 - k)
        sl[axis] = S - 1 - q if side else q
        debris[tuple(sl)] = 1
        q += 2 + k
    sl = [slice(None)] * 3
    sl[across] = 6
    sl[axis] = slice(S - 2, S) if side else slice(0, 2)
    fixed[tuple(sl)] = 1
    return debris, fixed


def interlocked(S, direction):
    """Two C shapes hooked into each other along the direction: each has a voxel ahead of a voxel of the other, a CYCLE of
    constraints (two pieces of one labelling never touch, so each link has one empty cell: D_A <= D_B + 1 <= D_A + 2).  B's
    lowest arm is 3 cells from the face, so D_B = 3 and D_A = 4: A closes the gap and both rest.  Returns debris."""
    axis, side = direction >> 1, direction & 1
    across = (axis + 1) % 3
    third = (axis + 2) % 3
    shape = np.zeros((S, S, S), np.uint8)

    def put(q, w):
        p = [0, 0, 0]
        p[axis], p[across], p[third] = (S - 1 - q if side else q), w, S // 2
        shape[tuple(p)] = 1
    # piece A (far from the face at w = 4 .. 6, q = 5 and 9, spine at w = 4); piece B the mirror image, hooked in
    for w in (4, 5, 6):
        put(9, w), put(5, w)
    for q in range(5, 10):
        put(q, 4)
    for w in (6, 7, 8):
        put(7, w), put(3, w)
    for q in range(3, 8):
        put(q, 8)
    return shape
