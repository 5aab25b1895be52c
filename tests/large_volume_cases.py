"""The cases of tests/test_gpu_volume_large.py: volumes large enough that three loops of the voxel-volume code take their
SECOND step -- the slot scan of the labelling (vrc_group.h: scan_slots, 1024 slots a step; 2048 slots at 256^3), the grid
stride of the one-box kernels (vrc_box_words.h: box_launch_groups, 16384 groups of 256; a whole-volume box at 512^3 is the
first to exceed them) and the stride over gridDim.y of the many-box kernels (vrc_volume.hip: split_for).  Beside the scenes
and their expected results: the launch geometry of those kernels restated in Python from the code as it stands, each with
the line it was read off, so that the host test (tests/test_volume_large_cases_host.py) can hold the cases to the regime
they are meant for.  box_word_items, item_words and the stride loop itself (walk) are posed_cases' restatements.  numpy
and Python integers only."""
import functools

import numpy as np

import components_model
import flood_model
import stamp_model
from posed_cases import box_word_items, item_words, walk            # vrc_box_words.h, restated once

NONE = components_model.NO_COMPONENT
GROUP = 256                          # lanes per workgroup of every kernel here
REPLACE, OR, ANDNOT = stamp_model.REPLACE, stamp_model.OR, stamp_model.ANDNOT


def apply_op(dst, bits, op):
    return bits if op == REPLACE else (dst | bits) if op == OR else (dst & (1 - bits))


# ---- the labelling's geometry ---------------------------------------------------------------------------------------

GROUP_KEYS = GROUP * 32              # vrc_components.hip:38-40: GROUP = 256, ROUNDS = 32, GROUP_KEYS = GROUP * ROUNDS
SCAN_GROUP = 1024                    # vrc_group.h, SCAN_GROUP: the slots scan_slots takes in one step


def groups_of(depth):
    """vrc_components.hip:249-253: workgroups of the labelling's kernels = slots of its scan"""
    return ((1 << (3 * depth)) + GROUP_KEYS - 1) // GROUP_KEYS


def scan_steps(n_slots):
    """vrc_group.h, the loop of scan_slots: for (base = 0; base < n_slots; base += SCAN_GROUP)"""
    return -(-n_slots // SCAN_GROUP)


def scan_slots(counts, carry=True):
    """vrc_group.h, scan_slots, on an array of counts: (the exclusive prefix, the total).  carry=False is for experiments with a
    wrong scan: one whose steps each start from zero"""
    counts = np.asarray(counts, np.int64)
    out = np.zeros_like(counts)
    running = total = 0
    for base in range(0, len(counts), SCAN_GROUP):
        step = counts[base:base + SCAN_GROUP]
        out[base:base + SCAN_GROUP] = running + np.cumsum(step) - step
        total = running + int(step.sum())
        running = total if carry else 0
    return out, total


def root_slots(rec, S):
    """the slot (workgroup of k_components_flatten) that counts each piece's root: its smallest key / GROUP_KEYS"""
    first = rec["first"].astype(np.int64)
    return components_model.keys(S)[first[:, 0], first[:, 1], first[:, 2]] // GROUP_KEYS


# ---- the one-box launch ---------------------------------------------------------------------------------------------

BOX_GROUPS = 16384                   # vrc_box_words.h:74: groups > 16384u ? 16384u : groups


def box_launch_groups(lo, hi):
    """vrc_box_words.h:71-75"""
    return min((box_word_items(lo, hi) + GROUP - 1) // GROUP, BOX_GROUPS)


def later_items(items, lanes):
    """the items a launch of `lanes` lanes takes after every lane's first, in the order of the loop
    for (it = lane; it < items; it += lanes) (k_fill_boxes, k_fill_spheres, k_copy_region, k_count_boxes of vrc_volume.hip; vrc_stamp.hip:70): walk's rows with iteration >= 1"""
    return np.arange(min(lanes, items), items, dtype=np.int64)


def second_lanes(items, lanes):
    """lanes that take a second item"""
    return max(0, min(items - lanes, lanes))


def words_of(lo, hi, Sd, which):
    """bool [cx, cy, kz] over the occupancy words of Sd^3 (2 x 2 x 8 voxels): the words the items `which` of the clipped box
    [lo, hi) are (row_word of vrc_box_words.h through posed_cases.item_words); items beyond their row's words are none"""
    n = Sd >> 1
    cx, cy, kz, valid = item_words(lo, hi, Sd)
    which = which[valid[which]]
    out = np.zeros((n, n, max(n >> 2, 1)), bool)
    out[cx[which], cy[which], kz[which]] = True
    return out


def differing_in(words, a, b):
    """the voxels at which the dense volumes a and b differ inside the words of the mask"""
    rows = np.flatnonzero(words.any(axis=(1, 2)))
    if not len(rows):
        return 0
    x0, x1 = 2 * int(rows[0]), 2 * int(rows[-1]) + 2
    S = a.shape[0]
    diff = a[x0:x1] != b[x0:x1]
    per_word = diff.reshape((x1 - x0) // 2, 2, S // 2, 2, S // 8, 8).sum(axis=(1, 3, 5))
    return int(per_word[words[x0 // 2:x1 // 2]].sum())


# ---- the many-box launch --------------------------------------------------------------------------------------------

def split_for(depth, n):
    """split_for of vrc_volume.hip: workgroups (gridDim.y) per box or sphere of a list of n in a volume of `depth`"""
    split = (4096 + n - 1) // n
    max_words = ((1 << (3 * depth)) // 8) // 4
    useful = (max_words + 255) // 256
    return max(1, min(split, 1024, useful))


def whole_box_items(depth):
    S = 1 << depth
    return box_word_items((0, 0, 0), (S, S, S))


# ---- scenes as lists of edits: the same list makes the dense array here and the volume on the device -----------------

def dense_of(edits, S):
    """edits: [("boxes", (n, 6), solid) | ("voxels", (n, 3), solid) | ("spheres", (n, 4), solid)] applied in order"""
    vol = np.zeros((S, S, S), np.uint8)
    for kind, items, solid in edits:
        items = np.asarray(items, np.int64)
        if kind == "boxes":
            for x0, y0, z0, x1, y1, z1 in items:
                vol[x0:x1, y0:y1, z0:z1] = solid
        elif kind == "voxels":
            vol[tuple(items.T)] = solid
        else:
            fill_spheres(vol, items, solid)
    return vol


def fill_spheres(vol, spheres, value):
    """dx^2 + dy^2 + dz^2 <= r^2 on an integer grid, over each sphere's clipped bounding box"""
    S = vol.shape[0]
    for cx, cy, cz, r in np.asarray(spheres, np.int64).tolist():
        lo = [max(0, c - r) for c in (cx, cy, cz)]
        hi = [min(S, c + r + 1) for c in (cx, cy, cz)]
        if r < 0 or any(l >= h for l, h in zip(lo, hi)):
            continue
        x, y, z = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r] = value


def sphere_box(S, sphere):
    """k_fill_spheres' clipped bounding box of (cx, cy, cz, r), or None (the head of the kernel in vrc_volume.hip)"""
    c, r = sphere[:3], sphere[3]
    lo = [max(0, int(v) - int(r)) for v in c]
    hi = [min(S, int(v) + int(r) + 1) for v in c]
    return None if r < 0 or any(l >= h for l, h in zip(lo, hi)) else (lo, hi)


def count_boxes(vol, boxes):
    S = vol.shape[0]
    out = []
    for b in np.asarray(boxes, np.int64).tolist():
        x0, y0, z0 = b[:3]
        x1, y1, z1 = [min(v, S) for v in b[3:]]
        out.append(int(vol[x0:x1, y0:y1, z0:z1].sum(dtype=np.int64)) if x0 < x1 and y0 < y1 and z0 < z1 else 0)
    return out


def random_boxes(rng, S, count, largest, smallest=1):
    lo = rng.integers(0, S - 2, (count, 3))
    return np.concatenate([lo, np.minimum(lo + rng.integers(smallest, largest + 1, (count, 3)), S)], axis=1).astype(np.uint32)


def plane_boxes(S, axis, pitch):
    """one-voxel slabs at every pitch-th coordinate of an axis, as boxes"""
    out = []
    for c in range(0, S, pitch):
        lo, hi = [0, 0, 0], [S, S, S]
        lo[axis], hi[axis] = c, c + 1
        out.append(lo + hi)
    return np.array(out, np.uint32)


# ---- 1. the labelling at 256^3, made of eight copies of a 128^3 part ---------------------------------------------------

def part_scene(h, seed=5):
    """h^3: the cells of a coarse random field as blocks of 4^3 (about a quarter of them), one voxel off the brick grid, with
    specks carved out of them and single voxels strewn between them; the outermost layer of every face is empty, so that
    copies set side by side do not touch, by corners either"""
    rng = np.random.default_rng(seed)
    coarse = (rng.random((h // 4,) * 3) < 0.25).astype(np.uint8)
    part = np.roll(coarse.repeat(4, 0).repeat(4, 1).repeat(4, 2), (1, 1, 1), (0, 1, 2))
    part[tuple(rng.integers(0, h, (h * h * h // 50, 3)).T)] = 0
    part[tuple(rng.integers(0, h, (h * h * h // 400, 3)).T)] = 1
    for face in (0, h - 1):
        part[face], part[:, face], part[:, :, face] = 0, 0, 0
    return part


OCTANTS = [(ox, oy, oz) for ox in (0, 1) for oy in (0, 1) for oz in (0, 1)]


def assemble(part, extras):
    """the part in every octant of (2h)^3, and the voxels `extras` (k, 3) set besides"""
    h = part.shape[0]
    vol = np.zeros((2 * h,) * 3, np.uint8)
    for ox, oy, oz in OCTANTS:
        vol[ox * h:(ox + 1) * h, oy * h:(oy + 1) * h, oz * h:(oz + 1) * h] = part
    assert not vol[tuple(np.asarray(extras).T)].any()
    vol[tuple(np.asarray(extras).T)] = 1
    return vol


def extras_for(part):
    """the voxels that join or mark the copies.  Across x = h - 1 | h, in each of the four pairs of octants: three bars of two
    voxels where the part is solid behind both ends (they merge a piece below key (2h)^3 / 2 with one above), one where
    it is solid behind the low end only (a piece that grows over the boundary) and one behind the high end only; a bar
    across the seam in y and one across the seam in z; and two specks with nothing around them, by corners either, in the
    last slot below the boundary (x = h - 1, y >= 2h - 16) and in the first above it (x = h, y < 16)"""
    h = part.shape[0]
    low, high = part[h - 2] != 0, part[1] != 0                # behind x = h - 1 from below, behind x = h from above
    out = []
    for kind, count in ((low & high, 3), (low & ~high, 1), (~low & high, 1)):
        yz = np.argwhere(kind)
        assert len(yz) >= 4 * count
        for j, (oy, oz) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            for y, z in yz[j::4][:count * 7:7].tolist():
                out += [(h - 1, y + oy * h, z + oz * h), (h, y + oy * h, z + oz * h)]
    x, z = np.argwhere((part[:, h - 2] != 0) & (part[:, 1] != 0))[5].tolist()
    out += [(x + h, h - 1, z), (x + h, h, z)]
    x, y = np.argwhere((part[:, :, h - 2] != 0) & (part[:, :, 1] != 0))[9].tolist()
    out += [(x, y + h, h - 1), (x, y + h, h)]
    # the specks: a seam voxel whose 26 neighbours are empty, the bars above included
    vol = assemble(part, np.array(out))
    near = flood_model.dilate(vol != 0, 26)
    for x, ys in ((h - 1, range(2 * h - 16, 2 * h - 1)), (h, range(1, 16))):
        free = [(x, y, z) for y in ys for z in range(1, 2 * h - 1) if not near[x, y, z]]
        out.append(free[len(free) // 2])
    return np.array(sorted(set(out)), np.int64)


def assembled_labelling(part, part_ids, extras, connectivity):
    """(ids, records) of assemble(part, extras) from the labelling `part_ids` of the part alone: the pieces of the eight
    copies and the extra voxels are the nodes of a union-find, united wherever an extra voxel has a neighbour; the classes
    are numbered by ascending smallest key (components_model.keys).  Right because the part's faces are empty: two copies,
    or a copy and anything else, meet only at an extra voxel"""
    h = part.shape[0]
    S = 2 * h
    for face in (0, h - 1):
        assert not part[face].any() and not part[:, face].any() and not part[:, :, face].any()
    C = int(part_ids[part_ids != NONE].max()) + 1
    node = np.full((S, S, S), -1, np.int64)
    local = np.where(part_ids == NONE, -1, part_ids.astype(np.int64))
    for o, (ox, oy, oz) in enumerate(OCTANTS):
        node[ox * h:(ox + 1) * h, oy * h:(oy + 1) * h, oz * h:(oz + 1) * h] = np.where(local < 0, -1, local + o * C)
    extras = np.asarray(extras, np.int64)
    assert (node[tuple(extras.T)] == -1).all()
    node[tuple(extras.T)] = 8 * C + np.arange(len(extras))
    parent = np.arange(8 * C + len(extras))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    steps = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (abs(dx) + abs(dy) + abs(dz) == 1 if connectivity == 6 else (dx, dy, dz) != (0, 0, 0))]
    for k, p in enumerate(extras.tolist()):
        for d in steps:
            q = [p[a] + d[a] for a in range(3)]
            if min(q) < 0 or max(q) >= S or node[q[0], q[1], q[2]] < 0:
                continue
            a, b = find(8 * C + k), find(int(node[q[0], q[1], q[2]]))
            parent[max(a, b)] = min(a, b)
    while True:
        up = parent[parent]
        if np.array_equal(up, parent):
            break
        parent = up
    K = components_model.keys(S)
    solid = node >= 0
    cls = parent[node[solid]]
    smallest = np.full(len(parent), np.int64(S) ** 3)
    np.minimum.at(smallest, cls, K[solid])
    reps = np.unique(smallest[cls])
    ids = np.full((S, S, S), NONE, np.uint32)
    ids[solid] = np.searchsorted(reps, smallest[cls]).astype(np.uint32)
    return ids, components_model.records_of(ids, K)


class Labelling:
    """vol, extras, and per connectivity (6, 26): ids, rec"""


@functools.lru_cache(maxsize=None)
def labelling_case(h=128):
    """eight copies of part_scene(h) with extras_for's bars and specks, and the expected labelling under both
    connectivities.  Shared by the tests: do not write to it."""
    case = Labelling()
    part = part_scene(h)
    case.part = part
    case.extras = extras_for(part)
    case.vol = assemble(part, case.extras)
    case.ids, case.rec = {}, {}
    for connectivity in (6, 26):
        part_ids, _ = components_model.label(part, connectivity)
        case.ids[connectivity], case.rec[connectivity] = assembled_labelling(part, part_ids, case.extras, connectivity)
    return case


def at_sample(case, connectivity, seed=3):
    """(n, 3) uint32: every root, the voxels of the two keys around the boundary S^3 / 2, (S/2 - 1, S - 1, S - 1) and (S/2, 0, 0),
    the corners, the extras and their neighbourhoods, the four layers around x = S / 2, and a random hundred thousand"""
    S = case.vol.shape[0]
    rng = np.random.default_rng(seed)
    e = S - 1
    special = [(S // 2 - 1, e, e), (S // 2, 0, 0)] + [(x, y, z) for x in (0, e) for y in (0, e) for z in (0, e)]
    around = (case.extras[:, None, :] + np.indices((3, 3, 3)).reshape(3, -1).T[None] - 1).reshape(-1, 3)
    slab = np.indices((4, S, S)).reshape(3, -1).T + [S // 2 - 2, 0, 0]
    xyz = np.concatenate([case.rec[connectivity]["first"].astype(np.int64), np.array(special), np.clip(around, 0, e), slab, rng.integers(0, S, (100000, 3))])
    return xyz.astype(np.uint32)


def keep_mask(case, connectivity, seed=4):
    """about half of the pieces, with the first and the last piece, the pieces of the bars and the specks kept, and the piece
    after each of them not"""
    rec = case.rec[connectivity]
    rng = np.random.default_rng(seed)
    keep = (rng.random(len(rec)) < 0.5).astype(np.uint8) * rng.integers(1, 256, len(rec)).astype(np.uint8)
    ids = case.ids[connectivity]
    forced = np.unique(np.concatenate([[0, len(rec) - 1], ids[tuple(case.extras.T)].astype(np.int64)]))
    keep[np.minimum(forced + 1, len(rec) - 1)] = 0
    keep[forced] = 1
    return keep


def content_edits(S):
    """something for select's OR and ANDNOT to meet: slabs at every third y"""
    return [("boxes", plane_boxes(S, 1, 3), 1)]


def serpentine_case(S=128):
    """flood_model.serpentine(S, 2): (vol, the one record it must label to).  S/2 layers of S/2 lines of S voxels, a voxel
    between two lines and one between two layers"""
    vol, start = flood_model.serpentine(S, 2)
    rec = np.zeros(1, components_model.RECORD)
    rec["first"], rec["lo"], rec["hi"] = start, (0, 0, 0), (S - 1, S - 1, S)
    rec["voxels"] = (S // 2) * ((S // 2) * S + S // 2 - 1) + S // 2 - 1
    return vol, rec


# ---- 2. one box at 512^3 --------------------------------------------------------------------------------------------

BIG = 512


def big_edits(which):
    """the two scenes of 512^3: slabs (every fifth z in the source, every third y in the destination), 150 random boxes set
    and 60 cleared, 300000 voxels set and 100000 cleared -- something in every word, nothing regular"""
    rng = np.random.default_rng(51200 + which)
    return [("boxes", plane_boxes(BIG, 2, 5) if which == 0 else plane_boxes(BIG, 1, 3), 1),
            ("boxes", random_boxes(rng, BIG, 150, 96), 1), ("boxes", random_boxes(rng, BIG, 60, 64), 0),
            ("voxels", rng.integers(0, BIG, (300000, 3)).astype(np.uint32), 1), ("voxels", rng.integers(0, BIG, (100000, 3)).astype(np.uint32), 0)]


@functools.lru_cache(maxsize=None)
def big_scene(which):
    """dense 512^3: 0 the source, 1 the destination.  Shared: do not write to it."""
    vol = dense_of(big_edits(which), BIG)
    vol.setflags(write=False)
    return vol


def copy_box(src_lo, size, dst_lo, Ss, Sd):
    """vrc_volume_copy_region's clipping (its loop over the axes in vrc_volume.hip): (lo, hi, offset) of the destination box, or None"""
    lo, hi, off = [], [], []
    for a in range(3):
        d0 = max(0, -dst_lo[a])
        d1 = min(size[a], Ss - src_lo[a], Sd - dst_lo[a])
        if d0 >= d1:
            return None
        lo.append(dst_lo[a] + d0)
        hi.append(dst_lo[a] + d1)
        off.append(src_lo[a] - dst_lo[a])
    return lo, hi, off


def copied(dst, src, src_lo, size, dst_lo, op):
    """a copy of dst after copyRegion(src, src_lo, size, dst_lo, op), by slices"""
    out = dst.copy()
    box = copy_box(src_lo, size, dst_lo, src.shape[0], dst.shape[0])
    if box is not None:
        lo, hi, off = box
        view = out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        view[...] = apply_op(view, src[lo[0] + off[0]:hi[0] + off[0], lo[1] + off[1]:hi[1] + off[1], lo[2] + off[2]:hi[2] + off[2]], op)
    return out


def shifted(dst, src, d, lo, hi, op):
    """stamp_model.stamp for the map q = p + d (m = the identity, t = d << 17) by slices: the box [lo, hi) of dst takes (op)
    src[p + d], 0 where that lies outside src"""
    out = dst.copy()
    Ss = src.shape[0]
    bits = np.zeros([hi[a] - lo[a] for a in range(3)], np.uint8)
    a0 = [max(lo[a], -d[a]) for a in range(3)]
    a1 = [min(hi[a], Ss - d[a]) for a in range(3)]
    if all(a0[a] < a1[a] for a in range(3)):
        bits[a0[0] - lo[0]:a1[0] - lo[0], a0[1] - lo[1]:a1[1] - lo[1], a0[2] - lo[2]:a1[2] - lo[2]] = \
            src[a0[0] + d[0]:a1[0] + d[0], a0[1] + d[1]:a1[1] + d[1], a0[2] + d[2]:a1[2] + d[2]]
    view = out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    view[...] = apply_op(view, bits, op)
    return out


# name: (src_lo, size, dst_lo, lanes that take a second word)
COPIES = {
    "whole": ((0, 0, 0), (BIG, BIG, BIG), (0, 0, 0), 65536),
    "unaligned": ((2, 0, 0), (BIG - 2, BIG - 2, BIG - 2), (1, 1, 1), 65536),        # [1, 511)^3 from one voxel further in x, one nearer in y and z
    "control": ((4, 0, 0), (BIG - 10, BIG - 2, BIG - 2), (3, 1, 1), 0),              # 252 brick rows in x: 16380 groups, one word a lane
}

TURN = ((2, 1, 0), (1, 1, 0))        # q = (S-1 - p_z, S-1 - p_y, p_x): a quarter turn about y and a mirror in y
PLACED_PIVOTS = ((256.0, 256.0, 256.0), (259.0, 251.0, 263.0))          # the source's middle lands 3, -5 and 7 voxels off the destination's
IDENTITY_ROT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def placed_case():
    """stampPlaced of the source at PLACED_PIVOTS without turning: (m, t, lo, hi, d) with d the whole-voxel shift the map is"""
    m, t, lo, hi = stamp_model.place(IDENTITY_ROT, 1.0, PLACED_PIVOTS[0], PLACED_PIVOTS[1], 9, 9)
    assert list(m) == stamp_model.IDENTITY[0] and all(v % (1 << 17) == 0 for v in t)
    return m, t, lo, hi, [v >> 17 for v in t]


def one_box_cases():
    """[(name, lo, hi, op, lanes that take a second word, before, after)] of every 512^3 launch of the GPU tests, dense.
    The arrays are made when asked for: before(), after()"""
    src, dst = big_scene(0), big_scene(1)
    S = BIG
    out = []
    for name, (src_lo, size, dst_lo, second) in COPIES.items():
        lo, hi, _ = copy_box(src_lo, size, dst_lo, S, S)
        for op in (REPLACE, OR):
            out.append(("copy " + name, lo, hi, op, second, lambda: dst, lambda a=(src_lo, size, dst_lo, op): copied(dst, src, *a)))
    whole = ([0, 0, 0], [S, S, S])
    out.append(("stamp identity", *whole, OR, 65536, lambda: dst, lambda: copied(dst, src, (0, 0, 0), (S, S, S), (0, 0, 0), OR)))
    out.append(("stamp turn", *whole, REPLACE, 65536, lambda: np.zeros_like(src), lambda: stamp_model.permuted(src, *TURN)))
    m, t, lo, hi, d = placed_case()
    out.append(("stamp placed", lo, hi, OR, 48896, lambda: dst, lambda: shifted(dst, src, d, lo, hi, OR)))
    return out


# ---- 3. many boxes at 64^3 ------------------------------------------------------------------------------------------

MANY_DEPTH = 6


@functools.lru_cache(maxsize=None)
def many_box_case():
    """64^3.  few: three boxes, the whole volume among them (split_for = 32: 8192 lanes for 9216 words).  many: 4100 random
    boxes of 12 to 40 voxels a side (split_for = 1: 256 lanes a box) and the whole volume last.  The spheres alike: one that
    covers the volume from its middle among three, and 4100 of radius 5 to 14"""
    S = 1 << MANY_DEPTH
    rng = np.random.default_rng(64)
    case = Labelling()
    case.base_edits = [("voxels", rng.integers(0, S, (20000, 3)).astype(np.uint32), 1)]
    case.few_boxes = np.array([[0, 0, 0, S, S, S], [1, 3, 5, S - 1, S - 4, S], [60, 61, 62, 70, 63, 0xFFFFFFFF]], np.uint32)
    case.many_boxes = np.concatenate([random_boxes(rng, S, 4100, 40, 12), [[0, 0, 0, S, S, S]]]).astype(np.uint32)
    case.few_spheres = np.array([[32, 31, 33, 60], [10, 50, 20, 12], [70, -3, 30, 15]], np.int32)
    case.many_spheres = np.concatenate([rng.integers(-5, S + 5, (4100, 3)), rng.integers(5, 15, (4100, 1))], axis=1).astype(np.int32)
    return case
