"""The cases of tests/test_gpu_volume_posed_large.py: a scene of 128^3 whose posed pieces make the kernels of vrc_rigid.hip that
gather them (k_place_affine, k_contacts, k_pair_contacts) take SEVERAL words a lane, and whose 257 pieces put the broad phase
(k_box_pairs) into a second workgroup.  Beside the generators: the launch geometry of those kernels restated in Python from
the code as it stands (vrc_box_words.h: box_word_items, row_word; vrc_rigid.hip: posed_grid and the stride loop), so that the
host test (tests/test_volume_posed_cases_host.py) can hold the cases to the regime they are meant for, and the models'
records computed from voxel lists in place of one dense array a piece (contact_model.record_at), which 257 pieces at 128^3
need to stay quick.  numpy and Python integers only."""
import functools

import numpy as np

import components_model
import contact_model
import pair_contact_model
import rigid_model
import stamp_model

NONE = components_model.NO_COMPONENT
GROUP = 256                     # lanes per workgroup (vrc_rigid.hip)
GRID_GROUPS = 16384             # workgroups of a posed launch, about
GRID_ROWS = 4096                # rows (pieces or pairs) of a posed launch, at most


# ---- the launch geometry, restated ------------------------------------------------------------------------------

def box_word_items(lo, hi):
    """box_word_items of vrc_box_words.h: brick rows in x times brick rows in y times the words a row touches at the most"""
    nbx = ((hi[0] - 1) >> 1) - (lo[0] >> 1) + 1
    nby = ((hi[1] - 1) >> 1) - (lo[1] >> 1) + 1
    wpr = (((((hi[2] - 1) >> 1) - (lo[2] >> 1)) + 3) >> 2) + 1
    return nbx * nby * wpr


def posed_grid(rows, Sd):
    """posed_grid of vrc_rigid.hip: (gridDim.x, gridDim.y) for `rows` pieces or pairs posed into Sd^3"""
    gy = min(rows, GRID_ROWS)
    whole = (box_word_items((0, 0, 0), (Sd, Sd, Sd)) + GROUP - 1) // GROUP
    return min(whole, GRID_GROUPS // gy), gy


def item_words(lo, hi, Sd):
    """row_word of vrc_box_words.h for every item of the clipped, non-empty box [lo, hi) of Sd^3 at once: (cx, cy, kz, valid) with
    kz the word's index within its brick row (cx, cy) and valid False where the row has fewer words than wpr"""
    n = Sd >> 1
    bx0, by0, cz0, cz1 = lo[0] >> 1, lo[1] >> 1, lo[2] >> 1, (hi[2] - 1) >> 1
    nby = ((hi[1] - 1) >> 1) - by0 + 1
    wpr = ((cz1 - cz0 + 3) >> 2) + 1
    it = np.arange(box_word_items(lo, hi), dtype=np.int64)
    k, row = it % wpr, it // wpr
    cx, cy = bx0 + row // nby, by0 + row % nby
    base = (cx * n + cy) * n
    w = ((base + cz0) >> 2) + k
    return cx, cy, w - (base >> 2), w <= ((base + cz1) >> 2)


def word_counts(points, Sd):
    """voxels of the (N, 3) list per occupancy word of Sd^3 (2 x 2 x 8 voxels), indexed [cx, cy, kz]"""
    n = Sd >> 1
    out = np.zeros((n, n, max(n >> 2, 1)), np.int64)
    p = np.asarray(points, np.int64).reshape(-1, 3)
    np.add.at(out, (p[:, 0] >> 1, p[:, 1] >> 1, p[:, 2] >> 3), 1)
    return out


def item_counts(points, box, Sd):
    """the posed voxels each item of `box` (lo + hi, clipped here) holds: what a lane adds to `posed` when it takes that item"""
    lo, hi = stamp_model.clip_box(Sd, box[:3], box[3:])
    cx, cy, kz, valid = item_words(lo, hi, Sd)
    return np.where(valid, word_counts(points, Sd)[cx, cy, np.where(valid, kz, 0)], 0)


def walk(items, gx, step_groups=None, iterations=None):
    """the stride loop of the posed kernels for one row of the grid: [(lane of the row, iteration, item)] as int64 columns, for
    base = blockIdx.x * GROUP; base < items; base += gridDim.x * GROUP.  step_groups and iterations are for experiments with a
    wrong loop: another stride, or only the first few iterations"""
    step = (gx if step_groups is None else step_groups) * GROUP
    lane = np.arange(gx * GROUP, dtype=np.int64)
    out = []
    trip = 0
    while (iterations is None or trip < iterations) and trip * step < items:
        it = lane + trip * step
        keep = it < items
        out.append(np.stack([lane[keep], np.full(int(keep.sum()), trip), it[keep]], 1))
        trip += 1
    return np.concatenate(out)


def carrying_lanes(points, box, gx, Sd):
    """(lanes that add posed voxels in at least two iterations, lanes that add any): the carry of sums from one stride
    iteration to the next that the large tests are about"""
    counts = item_counts(points, box, Sd)
    w = walk(len(counts), gx)
    busy = w[counts[w[:, 2]] > 0]
    per_lane = np.bincount(busy[:, 0], minlength=gx * GROUP)
    return int((per_lane >= 2).sum()), int((per_lane >= 1).sum())


# ---- the models' records from voxel lists ---------------------------------------------------------------------------

def posed_points(ids, i, mp, box, Sd):
    """the voxels of A_i (contact_model.posed) as an (N, 3) int64 list: stamp_model.source_bits over the clipped box alone"""
    if not rigid_model.map_legal(*mp):
        return np.zeros((0, 3), np.int64)
    box = (0, 0, 0, Sd, Sd, Sd) if box is None else [int(v) for v in box]
    clip = stamp_model.clip_box(Sd, box[:3], box[3:])
    if clip is None:
        return np.zeros((0, 3), np.int64)
    lo, hi = clip
    bits = stamp_model.source_bits((ids == i).astype(np.uint8), mp[0], mp[1], lo, hi)
    return np.argwhere(bits).astype(np.int64) + np.array(lo, np.int64)


def posed_point_sets(ids, maps, boxes, Sd, keep=None):
    """contact_model.posed_sets as voxel lists; None for a piece with keep[i] == 0"""
    return [None if keep is not None and not keep[i] else posed_points(ids, i, mp, None if boxes is None else boxes[i], Sd)
            for i, mp in enumerate(maps)]


def contacts_of(points, world):
    """contact_model.contacts from the voxel lists of posed_point_sets"""
    star = contact_model.walled(world)
    return [contact_model.record_at(() if p is None else p, star) for p in points]


def pair_records_of(points, pairs, Sd):
    """pair_contact_model.records_of from voxel lists: one W* at a time, filled and emptied again, the pairs taken by b"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = [None] * len(pairs)
    star = np.zeros((Sd + 2,) * 3, np.uint8)
    done = {}
    for b in sorted(set(pairs[:, 1].tolist())):
        rows = np.flatnonzero(pairs[:, 1] == b)
        if b >= len(points):
            for k in rows:
                out[k] = contact_model.ZERO
            continue
        at = None if points[b] is None or not len(points[b]) else tuple((points[b] + 1).T)
        if at is not None:
            star[at] = 1
        for k in rows:
            a = int(pairs[k, 0])
            if (a, b) not in done:
                done[a, b] = contact_model.ZERO if a >= len(points) or points[a] is None else contact_model.record_at(points[a], star)
            out[k] = done[a, b]
        if at is not None:
            star[at] = 0
    return out


# ---- the scene -------------------------------------------------------------------------------------------------------

def frame_and_blocks(S=128):
    """a lattice of one-voxel bars on a pitch of 16 -- ONE piece through the whole volume -- and blocks of 5 x 4 x 6 in its
    cells, on a pitch of 16 in x and y and 32 in z, none touching a bar: 257 pieces at 128^3 under 6-connectivity"""
    vol = np.zeros((S, S, S), np.uint8)
    vol[::16, :, ::16] = 1
    vol[:, ::16, ::16] = 1
    vol[::16, ::16, :] = 1
    for bx in range(4, S - 8, 16):
        for by in range(4, S - 8, 16):
            for bz in range(4, S - 8, 32):
                vol[bx:bx + 5, by:by + 4, bz:bz + 6] = 1
    return vol


def small_turn(rng, centre, target, half_size, Sd, reach=0.5):
    """pair_contact_model.turned_case's pose of one piece: a small turn about `centre`, which lands on `target`, and the box
    of the turned half_size, generous by two voxels"""
    ax, ay = rng.uniform(-reach, reach, 2)
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    inv = R.T
    m = [int(round(v * stamp_model.ONE)) for v in inv.reshape(9)]
    t = [int(round(v * (1 << 17))) for v in centre - inv @ target]
    half = np.abs(R) @ half_size + 2
    box = list(np.clip(np.floor(target - half), 0, Sd).astype(np.int64)) + list(np.clip(np.ceil(target + half), 0, Sd).astype(np.int64))
    return (m, t), box


class Case:
    """vol, ids, rec, maps [(m, t)], boxes (C, 6) uint32, keep (C,) uint8, base (a random 0.5 volume of the destination), Sd,
    frame (the lattice's index), whole (the blocks with the whole-volume box), odd (the rows with a box or a map of the odd kind)"""


FRAME_ROT = (0.5, 0.3)


@functools.lru_cache(maxsize=None)
def large_case(seed=11):
    """frame_and_blocks(128) posed into 128^3.  The frame under compose(rotation(0, 0.5), rotation(1, 0.3)) about the middle
    with the whole volume for a box; four blocks in different octants with the whole-volume box too; the other blocks under
    small turns, drawn towards the middle so that they meet the frame and each other, in boxes generous by two voxels; and
    rigid_model.pose_case's odd rows -- an empty box, an inverted one, one clipped by 0xFFFFFFFF, a map that reads 300 voxels
    outside the source -- with a keep mask of about 0.8 that keeps the frame, the four blocks and the last two pieces, so that
    the broad phase has runs on both sides of the boundary between its workgroups.  Shared by the tests: do not write to it."""
    S = Sd = 128
    rng = np.random.default_rng(seed)
    case = Case()
    case.vol = frame_and_blocks(S)
    case.ids, case.rec = components_model.label(case.vol, 6)
    case.Sd = Sd
    rec = case.rec
    C = len(rec)
    case.frame = int(np.argmax(rec["voxels"]))
    centres = (rec["lo"].astype(np.float64) + rec["hi"].astype(np.float64)) / 2
    whole = []
    for octant in (0, 3, 5, 6):                                             # the block nearest the middle of four octants
        want = np.array([32 + 64 * ((octant >> a) & 1) for a in range(3)], np.float64)
        order = np.argsort(np.abs(centres - want).sum(1))
        whole.append(int([i for i in order if i != case.frame][0]))
    case.whole = sorted(whole)
    maps, boxes = [], np.zeros((C, 6), np.uint32)
    for i in range(C):
        lo, hi = rec["lo"][i].astype(np.float64), rec["hi"][i].astype(np.float64)
        if i == case.frame:
            rot = stamp_model.compose(stamp_model.rotation(0, FRAME_ROT[0]), stamp_model.rotation(1, FRAME_ROT[1]))
            m, t, _, _ = stamp_model.place(rot, 1.0, (64, 64, 64), (64, 64, 64), 7, 7)
            maps.append((m, t))
            boxes[i] = [0, 0, 0, Sd, Sd, Sd]
            continue
        target = Sd / 2 + (centres[i] - S / 2) * 0.35 + rng.uniform(-1, 1, 3)
        mp, box = small_turn(rng, centres[i], target, (hi - lo) / 2, Sd)
        maps.append(mp)
        boxes[i] = [0, 0, 0, Sd, Sd, Sd] if i in case.whole else box
    plain = [i for i in range(C) if i != case.frame and i not in case.whole and i < C - 2]
    case.odd = dict(zip(("empty", "inverted", "clipped", "outside"), plain[5:9]))
    boxes[case.odd["empty"]] = [40, 40, 40, 40, 49, 49]
    boxes[case.odd["inverted"]] = [90, 30, 30, 50, 80, 80]
    boxes[case.odd["clipped"], 3:] = 0xFFFFFFFF
    i = case.odd["outside"]
    maps[i] = (maps[i][0], [v + (300 << 17) for v in maps[i][1]])
    keep = (rng.random(C) < 0.8).astype(np.uint8)
    keep[[case.frame] + case.whole + [C - 2, C - 1] + list(case.odd.values())] = 1
    case.maps, case.boxes, case.keep = maps, boxes, keep
    case.base = (rng.random((Sd, Sd, Sd)) < 0.5).astype(np.uint8)
    return case


@functools.lru_cache(maxsize=None)
def large_points(seed=11):
    """posed_point_sets of large_case(seed) with its boxes and keep mask, computed once"""
    case = large_case(seed)
    return posed_point_sets(case.ids, case.maps, case.boxes, case.Sd, case.keep)


@functools.lru_cache(maxsize=None)
def large_pairs(seed=11):
    """pair_contact_model.box_pairs of large_case(seed): the candidate list, computed once"""
    case = large_case(seed)
    return pair_contact_model.box_pairs(case.boxes, case.Sd, case.keep)


def boundary_window(pairs, boundary=GROUP):
    """(first, capacity) of a window of the candidate list that starts inside the run of a piece below `boundary` -- not at its
    first entry -- and ends inside the run of piece `boundary`, before its last entry: the two runs lie in different
    workgroups of k_box_pairs"""
    a = np.asarray(pairs)[:, 0].astype(np.int64)
    below, at = np.flatnonzero(a < boundary), np.flatnonzero(a == boundary)
    first = int(below[-1]) - 1
    return first, int(at[0]) + 2 - first


@functools.lru_cache(maxsize=None)
def scaled_case(seed=13):
    """labels of 64^3 posed into 128^3 at scale 2.  The 64^3 corner of frame_and_blocks(128) has the lattice and 32 blocks, too
    few for the grid to stride (61 rows at 128^3), so the free cells along z get a block as well and the middle of every cell a
    speck: 129 pieces.  The frame under the frame's turn of large_case and every other piece under a turn of its own, all
    through stamp_model.place with scale 2; boxes by rigid_model.place_box, the frame's the whole volume; a keep mask of
    about 0.8 that keeps the frame"""
    S, Sd = 64, 128
    rng = np.random.default_rng(seed)
    case = Case()
    vol = frame_and_blocks(128)[:S, :S, :S].copy()
    for bx in range(4, S - 8, 16):
        for by in range(4, S - 8, 16):
            for bz in range(20, S - 8, 32):
                vol[bx:bx + 5, by:by + 4, bz:bz + 6] = 1
    vol[12::16, 12::16, 12::16] = 1
    case.vol = vol
    case.ids, case.rec = components_model.label(vol, 6)
    case.Sd = Sd
    rec = case.rec
    C = len(rec)
    case.frame = int(np.argmax(rec["voxels"]))
    maps, boxes = [], np.zeros((C, 6), np.uint32)
    for i in range(C):
        lo, hi = rec["lo"][i], rec["hi"][i]
        if i == case.frame:
            rot = stamp_model.compose(stamp_model.rotation(0, FRAME_ROT[0]), stamp_model.rotation(1, FRAME_ROT[1]))
            m, t, _, _ = stamp_model.place(rot, 2.0, (32, 32, 32), (64, 64, 64), 6, 7)
            box = [0, 0, 0, Sd, Sd, Sd]
        else:
            centre = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
            rot = stamp_model.compose(stamp_model.rotation(0, rng.uniform(-0.5, 0.5)), stamp_model.rotation(int(rng.integers(1, 3)), rng.uniform(-0.5, 0.5)))
            target = Sd / 2 + (centre - S / 2) * 1.5 + rng.uniform(-1, 1, 3)
            m, t, blo, bhi = rigid_model.place_box(rot, 2.0, centre, target, lo, hi, 7)
            box = blo + bhi
        maps.append((m, t))
        boxes[i] = box
    keep = (rng.random(C) < 0.8).astype(np.uint8)
    keep[case.frame] = 1
    case.maps, case.boxes, case.keep = maps, boxes, keep
    case.base = (rng.random((Sd, Sd, Sd)) < 0.5).astype(np.uint8)
    return case
