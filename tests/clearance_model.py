"""The yardstick of the clearance tests (include/vrc.h: vrc_rigid_clearance), numpy and Python integers only.  ids are uint32
[x, y, z] arrays with NONE outside the pieces (components_model.label), fields dense uint32 [x, y, z] arrays with NONE for "no
value" (distance_model.field, travel_model.field), maps (m, t) pairs as in rigid_model.  A record is the tuple (posed, none,
sum, min_value, [min_at x3], max_value, [max_at x3]) of Python integers.  The posed set of a piece is contact_model.posed's, as
the voxel list posed_cases.posed_points makes of it (tests/test_volume_posed_cases_host.py holds the two against each other);
everything after it is brute force over the voxels of the set.  The case generators of the GPU tests live here so that the host
test can check them."""
import functools

import numpy as np

import components_model
import distance_model
import posed_cases
import rigid_model
import stamp_model
import travel_model

NONE = distance_model.NONE
EMPTY = (0, 0, 0, NONE, [0, 0, 0], 0, [0, 0, 0])                              # the record of the empty set


def voxel_of(index, S):
    """the voxel of dense index (x*S + y)*S + z"""
    return [int(index // (S * S)), int(index // S % S), int(index % S)]


def record(points, D):
    """the clearance record of the (N, 3) voxel list `points` over the dense field D"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    if not len(p):
        return EMPTY
    S = D.shape[0]
    value = D[tuple(p.T)].astype(np.int64)
    index = (p[:, 0] * S + p[:, 1]) * S + p[:, 2]
    finite = value != NONE
    if not finite.any():
        return (len(p), len(p)) + EMPTY[2:]
    value, index = value[finite], index[finite]
    lo, hi = int(value.min()), int(value.max())
    return (len(p), int(len(p) - len(value)), sum(value.tolist()), lo, voxel_of(index[value == lo].min(), S), hi, voxel_of(index[value == hi].min(), S))


def records_of(points, D):
    """one record per voxel list of posed_cases.posed_point_sets (None: a piece with keep[i] == 0)"""
    return [record(() if p is None else p, D) for p in points]


def clearance(ids, maps, boxes, D, keep=None):
    """one record per map: piece i posed by maps[i] inside boxes[i] (None: all of the field) into a volume of D's size"""
    return records_of(posed_cases.posed_point_sets(ids, maps, boxes, D.shape[0], keep), D)


def record_tuple(rec):
    """a capi.CLEARANCE_DTYPE record in the model's form; its reserved word must be 0"""
    assert int(rec["reserved"]) == 0
    return (int(rec["posed"]), int(rec["none"]), int(rec["sum"]), int(rec["min_value"]), [int(v) for v in rec["min_at"]],
            int(rec["max_value"]), [int(v) for v in rec["max_at"]])


def tuples(records):
    return [record_tuple(r) for r in records]


def free_radius(min_value, S):
    """VoxelLabels.freeRadius' rule for one value, from its definition: the largest r >= 0 with r^2 < min_value, by counting up"""
    if min_value == NONE:
        return S
    r = -1
    while (r + 1) ** 2 < min_value:
        r += 1
    return r


def translated(mp, o):
    """the map that poses the set of `mp` moved by the integer offset o: t'_a = t_a - 2 sum_c m[3a + c] o_c"""
    m, t = mp
    return (list(m), [int(t[a]) - 2 * sum(int(m[3 * a + c]) * int(o[c]) for c in range(3)) for a in range(3)])


def nearest_solid(world, p):
    """(the squared distance, the solid voxel of smallest dense index at that distance) from voxel p; the world is not empty"""
    solid = np.argwhere(world).astype(np.int64)                                # in dense-index order
    d2 = ((solid - np.asarray(p, np.int64)) ** 2).sum(1)
    k = int(np.argmin(d2))                                                     # the first of the least
    return int(d2[k]), [int(v) for v in solid[k]]


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------

def air_seed(world):
    """one seed volume for a travel field through the air: the first voxel of the largest 6-connected piece of the air, so that
    the field reaches much of it and leaves the solid and the air's other pieces at NONE"""
    _, rec = components_model.label(world, 6, True)
    seeds = np.zeros_like(world)
    seeds[tuple(rec["first"][int(np.argmax(rec["voxels"]))])] = 1
    return seeds


def fields_of(world):
    """the four fields of a world the random tests read: [(name, (to_empty, outside) or None for the travel field, dense field)]"""
    inside = distance_model.field(world)
    return [("solid", (False, False), inside), ("solid, open border", (False, True), distance_model.open_border(inside)),
            ("empty", (True, False), distance_model.field(world, True)), ("travel", None, travel_model.field(world, air_seed(world), 6, True))]


PLATE_BOX = [8, 14, 8, 56, 34, 56]


def plate_case(S=64):
    """a plate of 40 x 1 x 40 voxels at y = 20 over a floor slab y < 3 that fills x and z: (plate volume, world, maps, box).
    maps[0] is the identity: the whole plate is 18 voxels above the slab's top layer and every voxel holds 324.  maps[1] tilts
    it about z so that y falls as x grows, with the pivot's height chosen so that exactly ONE row of it along z, the last one in x,
    reaches the lowest layer: the least value lies in the last items of the box that hold a voxel, the greatest in the first.
    The box is generous so that its words span several workgroups."""
    plate = np.zeros((S, S, S), np.uint8)
    plate[10:50, 20, 12:52] = 1
    world = np.zeros((S, S, S), np.uint8)
    world[:, 0:3, :] = 1
    m, t, _, _ = stamp_model.place(stamp_model.rotation(2, -0.12), 1.0, (30, 20.5, 32), (30, 25.3125, 32), 6, 6)
    return plate, world, [(list(stamp_model.IDENTITY[0]), [0, 0, 0]), (m, t)], PLATE_BOX


def small_world_case(S):
    """the three pieces of test_a_world_of_4_cubed (tests/test_gpu_volume_contacts.py), a 16^3 labelling shrunk by point sampling
    into S^3, S = 4 or 8: by 4 into 4^3, where two brick rows share an occupancy word, by 2 into 8^3, where a row is one
    word.  Returns (debris, maps, boxes)."""
    debris = np.zeros((16, 16, 16), np.uint8)
    debris[0:9, 0:16, 0:7] = 1
    debris[10:16, 2:14, 0:16] = 1
    debris[0:8, 3:9, 9:16] = 1
    f = 16 // S
    shrink = [f * stamp_model.ONE if a == b else 0 for a in range(3) for b in range(3)]
    turned = [0, f * stamp_model.ONE, 0, -f * stamp_model.ONE, 0, 0, 0, 0, f * stamp_model.ONE]
    maps = [(shrink, [0, 0, 0]), (shrink, [-(3 << 17), 1 << 16, 0]), (turned, [0, 16 << 17, 5 << 15])]
    k = S // 4
    boxes = np.array([[0, 0, 0, S, S, S], [k, 0, 0, S, 3 * k, S], [0, 0, k, S, S, 0xFFFFFFFF]], np.uint32)
    return debris, maps, boxes


class Advance:
    """debris (16^3), ids, world (64^3), maps, D (the field to the solid, outside 0), records (the model's), rounds (16 x (C, 3)
    offsets), last ((C, 3) offsets onto the nearest solid voxel), reach ((C,) bool: |last|_inf <= 8)"""


REACH = 8


@functools.lru_cache(maxsize=None)
def advancement_case(seed):
    """Conservative advancement.  rigid_model.random_debris(16, seed) under general rotations about the middle of the 16^3
    volume, which lands within a voxel of the middle of a 64^3 world: every posed set lies within 8 sqrt(3) + 1.5 < 16 of it,
    inside [16, 48)^3, and a translation by |o|_inf <= 8 keeps it inside [8, 56)^3 -- nothing is ever clipped.  The world is a
    sparse random shell outside [12, 52)^3 and a few solid voxels inside.  Shared by the tests: do not write to it."""
    rng = np.random.default_rng(seed)
    case = Advance()
    case.debris = rigid_model.random_debris(16, seed)
    case.ids, rec = components_model.label(case.debris, 6)
    C = len(rec)
    S = 64
    world = (rng.random((S, S, S)) < 0.03).astype(np.uint8)
    world[12:52, 12:52, 12:52] = 0
    inner = rng.integers(14, 50, (48, 3))
    world[tuple(inner.T)] = 1
    case.world = world
    case.maps = []
    for _ in range(C):
        rot = stamp_model.compose(stamp_model.rotation(0, rng.uniform(0, 6.28)), stamp_model.rotation(int(rng.integers(1, 3)), rng.uniform(0, 6.28)))
        m, t, _, _ = stamp_model.place(rot, 1.0, (8, 8, 8), tuple(32 + rng.uniform(-1, 1, 3)), 4, 6)
        case.maps.append((m, t))
    case.D = distance_model.field(world)
    case.points = posed_cases.posed_point_sets(case.ids, case.maps, None, S)
    case.records = records_of(case.points, case.D)
    # the offsets of a round: every other piece from the whole reach, the rest short ones, so that both sides of
    # |o|^2 < min_value occur
    case.rounds = []
    for _ in range(16):
        o = rng.integers(-REACH, REACH + 1, (C, 3))
        short = rng.random(C) < 0.5
        o[short] = rng.integers(-2, 3, (int(short.sum()), 3))
        case.rounds.append(o.astype(np.int64))
    case.last = np.zeros((C, 3), np.int64)
    for i, r in enumerate(case.records):
        if r[0]:
            d2, q = nearest_solid(world, r[4])
            assert d2 == r[3]
            case.last[i] = np.array(q) - np.array(r[4])
    case.reach = np.array([r[0] > 0 for r in case.records]) & (np.abs(case.last).max(1) <= REACH)
    return case

