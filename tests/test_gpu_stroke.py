"""The capsule brush on the GPU (vrc_stroke_fill_capsules, vrc_stroke_fill_at_hits): every download is compared bit for bit
with the numpy model (stroke_model.py), setting and clearing, in the host and the device memory form; the centres of a stroke
come from the host function vrc_hit_to_voxel, the committed nodes from the host builder."""
import numpy as np
import pytest

import stroke_model as model
from stroke_model import gaps_of, mixed_items, scan_rays
from volume_support import Stream, committed, expected_nodes, same, volume_of

pytestmark = pytest.mark.gpu

LIMIT = 8192


def on_device(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def both_forms(volume, other, items, solid, stream):
    """the batch through the host form into `volume` and through the device form, on a created stream, into `other`"""
    items = np.ascontiguousarray(items, np.int32).reshape(-1, 8)
    volume.fillCapsules(items, solid)
    t = on_device(items)
    other.fillCapsulesDevice(len(items), t.data_ptr(), solid, stream)
    return t                                               # kept alive by the caller until the download has waited for the edit


# ---- 1. batches of mixed capsules ------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3, 5, 6])
def test_mixed_batches(built, depth):
    """depth 2: two brick rows share a word of the occupancy"""
    S = 1 << depth
    rng = np.random.default_rng(900 + depth)
    vol = (rng.random((S, S, S)) < 0.3).astype(np.uint8)
    volume, other = volume_of(vol), volume_of(vol)
    with Stream() as stream:
        for round_, solid in enumerate((True, False, True, False)):
            items = mixed_items(rng, S, 200 if round_ < 2 else 7)
            assert sum(model.kept(i) for i in items.tolist()) < len(items) or round_ >= 2
            keep = both_forms(volume, other, items, solid, stream)
            model.fill_capsules(vol, items, 1 if solid else 0)
            assert np.array_equal(volume.download(), vol), (depth, round_, "host form")
            assert np.array_equal(other.download(), vol), (depth, round_, "device form")      # download waits for the stream's edit
            del keep
    assert volume.solidCount() == int(vol.sum(dtype=np.int64))
    if depth >= 5:
        assert same(committed(volume), expected_nodes(vol, depth))


# ---- 2. ties ---------------------------------------------------------------------------------------------------------

def test_ties_are_inside(built):
    """voxels at distance exactly r from the axis -- offsets (3, 4, 0) with r = 5, (6, 8, 0) with r = 10 -- and at t exactly 0 and
    exactly L2, where the rule changes case"""
    depth, S = 6, 64
    vol = np.zeros((S, S, S), np.uint8)
    volume = volume_of(vol)
    items = np.array([[10, 20, 20, 40, 20, 20, 5, 0], [30, 12, 45, 30, 50, 45, 10, 0], [50, 50, 5, 50, 50, 30, 5, 0],
                      [3, 40, 40, 15, 49, 40, 5, 0]], np.int32)           # the last: d = (12, 9, 0), a 3-4-5 direction; (-3, 4, 0) is square to it
    volume.fillCapsules(items, True)
    model.fill_capsules(vol, items, 1)
    got = volume.download()
    assert np.array_equal(got, vol)
    for p in ((25, 23, 24), (25, 24, 17), (10, 23, 24), (40, 17, 16), (7, 20, 20), (45, 20, 20),       # r = 5 along x: square to it, t = 0, t = L2, the caps' poles
              (36, 30, 53), (22, 30, 39), (36, 12, 53), (24, 50, 37), (30, 2, 45), (30, 60, 45),        # r = 10 along y
              (53, 54, 17), (47, 50, 1), (53, 46, 30), (50, 50, 0), (50, 50, 35),                        # r = 5 along z
              (0, 44, 40), (6, 36, 40), (12, 53, 40), (18, 45, 40), (9, 44, 43)):                        # the slanted one: (-3, 4, 0) from a and from b
        assert got[p] == 1, p
    for p in ((25, 23, 25), (25, 25, 17), (9, 23, 24), (41, 17, 16), (4, 20, 20), (46, 20, 20), (36, 30, 54), (37, 12, 53), (30, 1, 45), (53, 54, 31),
              (50, 50, 36), (0, 45, 40), (19, 45, 40)):
        assert got[p] == 0, p
    volume.fillCapsules(items, False)
    assert volume.solidCount() == 0


# ---- 3. whole-word stores --------------------------------------------------------------------------------------------

def test_fat_capsule_builds_and_digs_whole_words(built):
    depth, S = 6, 64
    item = np.array([[20, 30, 26, 45, 35, 40, 20, 0]], np.int32)
    want = np.zeros((S, S, S), np.uint8)
    model.fill_capsules(want, item, 1)
    words = want.reshape(S // 2, 2, S // 2, 2, S // 8, 8).sum(axis=(1, 3, 5))
    assert (words == 32).sum() > 500 and ((words > 0) & (words < 32)).sum() > 500      # words stored whole, and words that take an atomic
    empty, full = volume_of(want * 0), volume_of(want * 0)
    full.fillBoxes([(0, 0, 0, S, S, S)], True)
    with Stream() as stream:
        keep = both_forms(empty, full, item, True, stream)
        assert np.array_equal(empty.download(), want) and full.solidCount() == S ** 3
        keep = both_forms(empty, full, item, False, stream)
        assert empty.solidCount() == 0 and np.array_equal(full.download(), 1 - want)
        del keep
    assert same(committed(full), expected_nodes(1 - want, depth))


# ---- 4. thin and long ------------------------------------------------------------------------------------------------

THIN = [(-40, -40, -40, 295, 295, 295), (0, 0, 0, 255, 1, 0), (0, 3, 250, 255, 254, 253),      # the first two have x as the major axis
        (5, 0, 7, 9, 255, 100), (250, 7, 0, 3, 60, 255)]                                        # y and z as the major axis


@pytest.mark.parametrize("r", [0, 1, 3])
def test_thin_and_long_at_256(built, r):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 8, 256
    assert [int(np.argmax(np.abs(np.array(t[3:]) - np.array(t[:3])))) for t in THIN[1:]] == [0, 0, 1, 2]
    empty, full = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
    full.fillBoxes([(0, 0, 0, S, S, S)], True)
    with Stream() as stream:
        for ends in THIN:
            item = np.array([list(ends) + [r, 0]], np.int32)
            want = np.zeros((S, S, S), np.uint8)
            model.fill_capsules(want, item, 1, sparse=True)
            assert want.sum() >= 2
            keep = both_forms(empty, full, item, True, stream)
            assert np.array_equal(empty.download(), want), (ends, r)
            keep = both_forms(empty, full, item, False, stream)
            assert empty.solidCount() == 0, (ends, r)
            got = full.download()
            assert np.array_equal(got, 1 - want), (ends, r)
            keep = both_forms(empty, full, item, True, stream)                 # back to empty and full for the next
            empty.fillCapsules(item, False)
            assert full.solidCount() == S ** 3
            del keep


def test_whole_diagonal_at_512(built):
    """one capsule over 32 pieces with split_for's 1024 workgroups: blockIdx.y strides over the pieces' words"""
    import cpuvoxelraycaster_amd as vrc
    depth, S = 9, 512
    item = np.array([[0, 0, 0, S - 1, S - 1, S - 1, 2, 0]], np.int32)
    p = model.capsule_voxels_sparse(S, item[0].tolist())
    volume = vrc.VoxelVolume(depth)
    volume.fillCapsules(item, True)
    assert volume.solidCount() == len(p) > 5 * S
    got = volume.download()
    assert got[p[:, 0], p[:, 1], p[:, 2]].all() and int(got.sum(dtype=np.int64)) == len(p)       # exactly the model's voxels
    t = on_device(item)
    with Stream() as stream:
        volume.fillCapsulesDevice(1, t.data_ptr(), False, stream)
        assert volume.solidCount() == 0


# ---- 5. many short capsules ------------------------------------------------------------------------------------------

def records_at(cells, S, miss_every=0):
    """hit records whose voxel is cells[i] (the centre of the point-reflected cell, exact in float32 for S <= 128), normal
    (0, -2, 0): the neighbour is y + 1; every miss_every-th record is a miss"""
    import cpuvoxelraycaster_amd as vrc
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    rec = np.zeros(len(cells), vrc.HIT_DTYPE)
    rec["hit"] = 1
    if miss_every:
        rec["hit"][miss_every - 1::miss_every] = 0
    rec["position"] = (1.0 + (S - 1 - cells + 0.5) / S).astype(np.float32)
    rec["normal"][:, 1] = -2
    return rec


def test_five_thousand_short_capsules(built):
    """one call of 5000: a workgroup per capsule (split_for gives 1); through the hits form with radius <= 4, a wave per capsule"""
    import cpuvoxelraycaster_amd as vrc
    depth, S = 7, 128
    rng = np.random.default_rng(5000)
    a = rng.integers(-2, S + 2, (5000, 3))
    step = rng.integers(-3, 4, (5000, 3))                                      # length <= sqrt(27) < 6
    items = np.concatenate([a, a + step, rng.integers(0, 4, (5000, 1)), np.zeros((5000, 1), np.int64)], axis=1).astype(np.int32)
    vol = (rng.random((S, S, S)) < 0.2).astype(np.uint8)
    scene = vrc.LSVO.fromVolume(vol, depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    other = volume.clone()
    with Stream() as stream:
        keep = both_forms(volume, other, items[:2500], True, stream)
        model.fill_capsules(vol, items[:2500], 1)
        keep2 = both_forms(volume, other, items, False, stream)
        model.fill_capsules(vol, items, 0)
        assert np.array_equal(volume.download(), vol) and np.array_equal(other.download(), vol)
        del keep, keep2
    # a random walk of 5000 records, steps up to 3 a coordinate, a miss at every 17th: the one-wave launch of the hits form
    walk = np.clip(np.cumsum(rng.integers(-3, 4, (5000, 3)), axis=0) + S // 2, 0, S - 1)
    rec = records_at(walk, S, 17)
    for solid, radius, max_gap in ((True, 3, 0), (False, 2, 4)):
        centres, valid = model.hit_centres(depth, rec, solid)
        assert 3000 < valid.sum() < 4800                                     # the misses, and for a build the records at y = S - 1
        volume.strokeAtHits(rec, radius, solid, max_gap)
        t = on_device(rec)
        with Stream() as stream:
            other.strokeAtHitsDevice(len(rec), t.data_ptr(), radius, solid, max_gap, stream)
            model.fill_capsules(vol, model.stroke_items(centres, valid, radius, max_gap), 1 if solid else 0)
            assert np.array_equal(volume.download(), vol), (solid, radius, max_gap)
            assert np.array_equal(other.download(), vol), (solid, radius, max_gap)


# ---- 6. strokes through the hits of a ray batch ----------------------------------------------------------------------

@pytest.mark.parametrize("depth", [6, 7])
def test_stroke_at_hits_is_the_model(built, heights, depth):
    import torch
    import cpuvoxelraycaster_amd as vrc
    from volume_support import terrain_volume
    S = 1 << depth
    scene = vrc.LSVO.fromTerrain(heights, depth)
    terrain = terrain_volume(heights, depth)
    org, d = scan_rays(depth, 160, 2.5)
    hits = scene.castRays(org, d)
    kind = hits["hit"] & 0xff
    assert (kind == 1).sum() >= 100 and (kind == 0).sum() >= 12
    t_org, t_dir = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    t_hits = torch.zeros(len(org) * 12, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        for solid in (False, True):
            centres, valid = model.hit_centres(depth, hits, solid)
            gaps = gaps_of(centres, valid)
            print("depth %d %s: %d centres of %d records, %d links, steps %.1f .. %.1f voxels, %d above 4" %
                  (depth, "build" if solid else "dig", valid.sum(), len(valid), len(gaps), gaps.min(), gaps.max(), (gaps > 4).sum()))
            assert gaps.min() <= 1.0 and gaps.max() >= 6.0 and (gaps > 4).sum() >= 5 and (gaps <= 4).sum() >= 5 and (~valid).sum() >= 12
            for max_gap in (0, 1, 4):
                for radius in (0, 3):
                    vol = terrain.copy()
                    model.fill_capsules(vol, model.stroke_items(centres, valid, radius, max_gap), 1 if solid else 0)
                    assert (vol != terrain).sum() > 50
                    volume = vrc.VoxelVolume.fromScene(scene)
                    volume.strokeAtHits(hits, radius, solid, max_gap)
                    assert np.array_equal(volume.download(), vol), (depth, solid, max_gap, radius, "host form")
                    # the device form directly behind the cast, on the same stream, nothing in between
                    device = vrc.VoxelVolume.fromScene(scene)
                    scene.castRaysDevice(len(org), t_org.data_ptr(), t_dir.data_ptr(), t_hits.data_ptr(), stream=stream)
                    device.strokeAtHitsDevice(len(org), t_hits.data_ptr(), radius, solid, max_gap, stream)
                    assert np.array_equal(device.download(), vol), (depth, solid, max_gap, radius, "device form")
                    if (max_gap, radius) == (4, 3):
                        assert same(committed(device), expected_nodes(vol, depth))       # the commit after a stroke
                    volume.close()
                    device.close()


def test_stroke_leaves_one_tunnel_where_balls_leave_cavities(built, heights):
    """hits about 7 voxels apart, r = 2: what strokeAtHits digs is one 6-connected piece, what fillSpheresAtHits digs on the same
    hits is a string of separate ones.  What is dug is the SOLID part of the tunnel, so the path runs over ground whose relief
    between two hits stays within the radius: a link that crosses open air leaves its two ends apart, as it should"""
    import cpuvoxelraycaster_amd as vrc
    from volume_support import terrain_volume
    depth = 7
    scene = vrc.LSVO.fromTerrain(heights, depth)
    org, d = scan_rays(depth, 24, 7.0, varied=False, start=(20.5, 110.5))
    keep = np.ones(len(org), bool)
    keep[12::13] = False                                                       # no misses: one stroke
    hits = scene.castRays(org[keep], d[keep])
    centres, valid = model.hit_centres(depth, hits, False)
    gaps = gaps_of(centres, valid)
    assert valid.all() and len(gaps) == 22 and gaps.min() > 5.0 and gaps.max() < 16.0, (valid.sum(), gaps.min(), gaps.max())
    before = terrain_volume(heights, depth)
    pieces = {}
    for name in ("stroke", "balls"):
        volume = vrc.VoxelVolume.fromScene(scene)
        if name == "stroke":
            volume.strokeAtHits(hits, 2, False)
        else:
            volume.fillSpheresAtHits(hits, 2, False)
        dug = before ^ volume.download()
        assert dug.sum() > 0 and not (dug & ~before).any()
        medium = volume_of(dug)
        labels = medium.labelComponents(6, False)
        pieces[name] = labels.count
        labels.close()
        medium.close()
        volume.close()
    print("pieces dug:", pieces)
    assert pieces["stroke"] == 1 and pieces["balls"] >= 10


# ---- 7. at the limits of the 32-bit claims ---------------------------------------------------------------------------
# vrc_stroke.hip takes q.q, L2 and t as 32-bit values and multiplies 32 x 32 -> 64: right for items inside LIMIT in a volume
# of at most 1024^3.  The yardstick is the int64 model: q.q L2 < 2.6e8 * 8.1e8 and r^2 L2 < 6.8e7 * 8.1e8, both inside
# int64; each case also holds a sample of the model's voxels next to its surface to rule_int, which has no width at all.

def limit_cases(S):
    """{group: [item]} for a volume of S^3 = 64^3"""
    L = LIMIT
    signs = [(1, 1, 1), (1, -1, 1), (1, 1, -1), (1, -1, -1)]
    diagonals = [[-L * s[0], -L * s[1], -L * s[2], L * s[0], L * s[1], L * s[2], r, 0] for s in signs for r in (0, 3, 40)]
    # the same lines moved k = S + 2 voxels along x: they pass through (k, 0, 0), two voxels outside the volume, so the
    # lattice points themselves (r = 0) miss it; both ends stay inside the limit
    k = S + 2
    shifted = [[-L + k, -L * s[1], -L * s[2], L, (L - k) * s[1], (L - k) * s[2], r, 0] for s in signs for r in (3, 40)]
    huge = []
    for r in (8000, L):
        # the unit vector (2, 3, 6) / 7: a centre r away from the volume's middle along it, so the surface crosses the volume as
        # a nearly flat slanted sheet; u = (-3, 2, 0) is square to it
        c = [S // 2 + (r * n + 3) // 7 for n in (2, 3, 6)]
        huge.append(c + c + [r, 0])                                            # the ball
        huge.append(c + [c[0] - 3 * 2300, c[1] + 2 * 2300, c[2], r, 0])        # the volume at the cap of end a (t <= 0 and t > 0 meet there)
        huge.append([c[0] + 3 * 1000, c[1] - 2 * 1000, c[2], c[0] - 3 * 2300, c[1] + 2 * 2300, c[2], r, 0])      # ... and beside the cylinder
        fore, back = (L - c[0]) // 3, (L - c[1]) // 2                          # the same axis as long as the limit lets it be: r^2 L2 > 2^53
        huge.append([c[0] + 3 * fore, c[1] - 2 * fore, c[2], c[0] - 3 * back, c[1] + 2 * back, c[2], r, 0])
    medium = [[-20, 10, 5, 90, 50, 70, 30, 0], [70, 60, -8, -9, 3, 66, 31, 0]]      # most words pass the pre-test `near`, many are whole
    return dict(diagonals=diagonals, shifted=shifted, huge=huge, medium=medium)


def surface_sample(want, rng, count=200):
    """about `count` voxels next to the surface of the model's set: both sides of it"""
    edge = np.zeros(want.shape, bool)
    for axis in range(3):
        step = np.diff(want.astype(np.int8), axis=axis) != 0
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        edge[tuple(lo)] |= step
        edge[tuple(hi)] |= step
    at = np.argwhere(edge)
    return at[rng.permutation(len(at))[:count]]


@pytest.mark.parametrize("group", ["diagonals", "shifted", "huge", "medium"])
def test_capsules_at_the_arithmetic_limits(built, group):
    depth, S = 6, 64
    rng = np.random.default_rng(64)
    empty_h, empty_d, full_h, full_d = (volume_of(np.zeros((S, S, S), np.uint8)) for _ in range(4))
    for volume in (full_h, full_d):
        volume.fillBoxes([(0, 0, 0, S, S, S)], True)
    with Stream() as stream:
        for item in limit_cases(S)[group]:
            assert model.kept(item), item
            want = model.fill_capsules(np.zeros((S, S, S), np.uint8), [item], 1)
            count = int(want.sum())
            print(group, item, count)
            assert 0 < count < S ** 3, item                                    # some, not all
            sample = surface_sample(want, rng)
            assert len(sample) >= min(200, count) and all(model.rule_int(p, item) == bool(want[tuple(p)]) for p in sample), item
            items = np.array([item], np.int32)
            keep = both_forms(empty_h, empty_d, items, True, stream)
            assert np.array_equal(empty_h.download(), want), (item, "set, host form")
            assert np.array_equal(empty_d.download(), want), (item, "set, device form")
            keep = both_forms(full_h, full_d, items, False, stream)
            assert np.array_equal(full_h.download(), 1 - want), (item, "cleared, host form")
            assert np.array_equal(full_d.download(), 1 - want), (item, "cleared, device form")
            keep = both_forms(empty_h, empty_d, items, False, stream)          # back to empty and full for the next
            keep = both_forms(full_h, full_d, items, True, stream)
            assert empty_h.solidCount() == empty_d.solidCount() == 0 and full_h.solidCount() == full_d.solidCount() == S ** 3, item
            del keep


def test_corner_to_corner_of_the_limit_at_the_largest_depth(built):
    """depth 10, the largest VoxelVolume accepts and the one the kernel's comment assumes: the only place where |q| on an axis
    exceeds 8192 + 64.  No download: the count, every voxel of the model and every 6-neighbour outside it"""
    import cpuvoxelraycaster_amd as vrc
    depth, S = 10, 1024
    L = LIMIT
    items = np.array([[-L, -L, -L, L, L, L, 2, 0], [L, -L, -L, -L, L, L, 2, 0]], np.int32)          # the second: mirrored in x
    cells = [model.capsule_voxels_sparse(S, item.tolist()) for item in items]
    assert len(cells[0]) > 5 * S and 0 < len(cells[1]) < 100                  # the mirrored one meets the volume at its corner alone
    field = np.unique(np.concatenate(cells), axis=0)
    key = lambda p: (p[:, 0] * S + p[:, 1]) * S + p[:, 2]
    around = np.concatenate([field + step for step in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))])
    around = around[np.all((around >= 0) & (around < S), axis=1)]
    around = np.unique(around[~np.isin(key(around), key(field))], axis=0)
    assert len(around) > len(field) // 2
    volume = vrc.VoxelVolume(depth)
    volume.fillCapsules(items, True)
    assert volume.solidCount() == len(field)
    assert volume.getVoxels(field.astype(np.uint32)).all() and not volume.getVoxels(around.astype(np.uint32)).any()
    t = on_device(items)
    with Stream() as stream:
        volume.fillCapsulesDevice(len(items), t.data_ptr(), False, stream)
        assert volume.solidCount() == 0
    volume.close()


def spanning(rng, S, count, radii):
    """capsules from one face of the volume, or beyond it, to the opposite one, along a seeded major axis"""
    a, b = rng.integers(0, S, (count, 3)), rng.integers(0, S, (count, 3))
    major = rng.integers(0, 3, count)
    a[np.arange(count), major] = -rng.integers(0, 20, count)
    b[np.arange(count), major] = S - 1 + rng.integers(0, 20, count)
    flip = rng.random(count) < 0.5
    a[flip], b[flip] = b[flip], a[flip].copy()
    return np.concatenate([a, b, rng.choice(radii, (count, 1)), np.zeros((count, 1), np.int64)], axis=1).astype(np.int32)


@pytest.mark.parametrize("depth,count,long", [(7, 5000, 300), (8, 300, 40)])
def test_long_capsules_in_a_large_batch(built, depth, count, long):
    """5000 at 128^3: split_for gives each capsule ONE workgroup, and a spanning one has 8 pieces or 9 -- the k += k_step loop
    runs that many rounds.  300 at 256^3: 14 workgroups for the 16 to 18 pieces of a spanning one, which do not divide"""
    S = 1 << depth
    rng = np.random.default_rng(depth * 1000 + count)
    a = rng.integers(-2, S + 2, (count, 3))
    items = np.concatenate([a, a + rng.integers(-3, 4, (count, 3)), rng.integers(0, 4, (count, 1)), np.zeros((count, 1), np.int64)], axis=1).astype(np.int32)
    where = rng.permutation(count)[:long]
    items[where] = spanning(rng, S, long, [0, 1, 3])
    vol = (rng.random((S, S, S)) < 0.2).astype(np.uint8)
    volume = volume_of(vol)
    other = volume.clone()
    with Stream() as stream:
        for solid in (True, False):
            keep = both_forms(volume, other, items, solid, stream)
            model.fill_capsules(vol, items, 1 if solid else 0, sparse=True)
            assert np.array_equal(volume.download(), vol), (depth, solid, "host form")
            assert np.array_equal(other.download(), vol), (depth, solid, "device form")
            del keep
            items = items[rng.permutation(len(items))[:len(items) // 2]]      # the clearing call: half of them, so that something stays
    assert volume.solidCount() == int(vol.sum(dtype=np.int64))
