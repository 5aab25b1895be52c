"""Voronoi fracture on the GPU (vrc_fracture_label, vrc_fracture_piece_sites; VoxelVolume.fracture / shatter,
VoxelLabels.pieceSites).  The expected result is the numpy model of tests/fracture_model.py (held against a literal loop and
a breadth-first search in tests/test_volume_fracture_host.py).  Every comparison is exact: the id at ALL S^3 coordinates,
every record and every piece's site."""
import itertools

import numpy as np
import pytest

import components_model
import fall_model
import fracture_model as model
from test_gpu_volume_components import Stream, all_coordinates, volume_of

pytestmark = pytest.mark.gpu

NONE = model.NONE


def check_labels(labels, ids, rec, sites, what):
    """count, records, at() of everything, the pieces' sites and the bytes held against an expected labelling"""
    S = ids.shape[0]
    assert labels.count == len(rec), (what, labels.count, len(rec))
    got = labels.components()
    for field in ("first", "lo", "hi", "reserved", "voxels"):
        assert np.array_equal(got[field], rec[field]), (what, field)
    at = labels.at(all_coordinates(S))
    assert np.array_equal(at[:S ** 3].reshape(S, S, S), ids), what
    assert (at[S ** 3:] == NONE).all(), what
    ps = labels.pieceSites()
    assert ps.dtype == np.uint32 and np.array_equal(ps, sites), what
    assert labels.bytes() == 4 * S ** 3 + 52 * len(rec)


def cells_of(labels, S):
    """the cell of every voxel of M, read through the voxel's piece"""
    at = labels.at(all_coordinates(S))[:S ** 3]
    ps = np.append(labels.pieceSites(), np.uint32(NONE))
    return ps[np.where(at == NONE, len(ps) - 1, at)].reshape(S, S, S)


def device_cells(S, sites, max_distance=None):
    """the cell of EVERY voxel: an empty medium through its empty voxels, so M is the whole volume"""
    import cpuvoxelraycaster_amd as vrc
    depth = S.bit_length() - 1
    empty = vrc.VoxelVolume(depth)
    labels = empty.fracture(sites, 6, True, max_distance)
    empty.close()
    assert int(labels.components()["voxels"].sum()) == S ** 3
    cell = cells_of(labels, S)
    labels.close()
    return cell


def random_sites(rng, S, n):
    """n sites, some outside the volume and some duplicated"""
    sites = rng.integers(-2, S + 2, (n, 3))
    if n > 2:
        sites[n // 2] = sites[0]
        sites[n - 1] = sites[1]
    return sites.astype(np.int32)


# ---- random media and random sites ------------------------------------------------------------------------------

SITE_COUNTS = (1, 2, 7, 200)
RADII = (None, 0, 3, 10)                      # max_d2 unlimited, 0, 9, 100


@pytest.mark.parametrize("through_empty", [False, True])
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_random_media_and_sites(built, depth, connectivity, through_empty):
    """Depth 2 is the two-word volume, depth 6 the first with two bit-words per column and columns of one whole wave.  Up to
    32^3 every site count meets every cut-off; at 64^3 each of the four (connectivity, through) cases takes another diagonal of
    that square, so the four together cover it."""
    S = 1 << depth
    k = (connectivity == 26) * 2 + int(through_empty)
    rng = np.random.default_rng(9000 + 100 * depth + 10 * k)
    in_m = rng.random((S, S, S)) < (0.55 if connectivity == 6 else 0.3)
    vol = (~in_m if through_empty else in_m).astype(np.uint8)
    volume = volume_of(vol, depth)
    pairs = [(n, r) for n in SITE_COUNTS for r in RADII] if depth < 6 else [(SITE_COUNTS[i], RADII[(i + k) % 4]) for i in range(4)]
    for n, r in pairs:
        sites = random_sites(rng, S, n)
        if n == 1:
            sites[0] = rng.integers(0, S, 3)
        ids, rec, ps = model.label(vol, sites, connectivity, through_empty, NONE if r is None else r * r)
        labels = volume.fracture(sites, connectivity, through_empty, r)
        check_labels(labels, ids, rec, ps, (depth, connectivity, through_empty, n, r))
        assert int(rec["voxels"].sum()) == int(in_m.sum())
        labels.close()
    volume.close()


# ---- ties -------------------------------------------------------------------------------------------------------

def tie_cases(S):
    """(name, coordinates) around the middle of the volume; every distance between two of them along an axis is even"""
    c, h = S // 2 - 1, 2 if S == 8 else 6
    cases = []
    for a in range(3):
        p = [[c, c, c], [c, c, c]]
        p[0][a], p[1][a] = c - h, c + h
        cases.append((f"pair along {'xyz'[a]}", p))                       # the plane at c goes to the lower index
    for a in range(3):
        square = []
        for u, v in itertools.product((c - h, c + h), repeat=2):
            q = [c + 1, c + 1, c + 1]
            q[(a + 1) % 3], q[(a + 2) % 3] = u, v
            square.append(q)
        cases.append((f"square across {'xyz'[a]}", square))
    cases.append(("cube", [list(q) for q in itertools.product((c - h, c + h), repeat=3)]))      # the centre is equidistant from all
    cases.append(("one z column", [[c, c, c - 1], [c, c, c + 1]]))       # (c, c, c) lies between them
    for a in range(3):
        # a collinear triple along `a` whose middle site stands h aside: along the line through the outer two, the
        # parabolas are (i - c + h)^2, h^2 + (i - c)^2 and (i - c - h)^2 -- all three are h^2 at i = c, and the middle one
        # is lowest nowhere else.  The voxel it can only win by a tie is (c, c, c); a pop on >= loses it.
        t = [[c, c, c], [c, c, c], [c, c, c]]
        t[0][a], t[2][a] = c - h, c + h
        t[1][(a + 1) % 3] = c + h
        cases.append((f"triple along {'xyz'[a]}", t))
    cases.append(("duplicates", [[c, c, c], [c, c, c], [c + 2, c, c], [c + 2, c, c]]))
    return cases


def orders_of(n):
    """every permutation up to four sites; of the cube's 40320 its 16 rotations and reflections of the index cycle and 24
    drawn at random -- the lowest index visits every corner"""
    if n <= 4:
        return list(itertools.permutations(range(n)))
    base = list(range(n))
    turns = [base[k:] + base[:k] for k in range(n)]
    rng = np.random.default_rng(40320)
    return [tuple(t) for t in turns] + [tuple(t[::-1]) for t in turns] + [tuple(rng.permutation(n)) for _ in range(24)]


@pytest.mark.parametrize("S", [8, 32])
def test_ties_go_to_the_lowest_index(built, S):
    for name, coords in tie_cases(S):
        coords = np.array(coords, np.int32)
        assert coords.min() >= 0 and coords.max() < S
        tied = 0
        for order in orders_of(len(coords)):
            sites = coords[list(order)]
            want = model.cells(S, sites)
            got = device_cells(S, sites)
            assert np.array_equal(got, want), (S, name, order, np.argwhere(got != want)[:4].tolist())
        # the case does tie: some voxel has more than one nearest site
        c = np.arange(S, dtype=np.int64)
        d2 = np.stack([((c - x) ** 2)[:, None, None] + ((c - y) ** 2)[None, :, None] + ((c - z) ** 2)[None, None, :] for x, y, z in coords])
        tied = int(((d2 == d2.min(axis=0)).sum(axis=0) > 1).sum())
        assert tied > 0, name
        print(f"{S}^3 {name}: {len(orders_of(len(coords)))} orders, {tied} voxels with several nearest sites")


def test_the_triple_s_tie_voxel(built):
    """by hand at 8^3: the sites (1, 3, 3), (4, 6, 3) and (7, 3, 3) are all 9 away from the voxel (4, 3, 3), and along the x line
    through it the middle site's parabola is lowest nowhere else: the voxel goes to index 0, whichever site carries it"""
    coords = np.array([[1, 3, 3], [4, 6, 3], [7, 3, 3]], np.int32)
    for order in itertools.permutations(range(3)):
        sites = coords[list(order)]
        assert device_cells(8, sites)[4, 3, 3] == 0, order


# ---- reductions to known results --------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [6, 26])
def test_reductions(built, connectivity):
    depth, S = 5, 32
    rng = np.random.default_rng(321 + connectivity)
    vol = (rng.random((S, S, S)) < (0.3 if connectivity == 6 else 0.12)).astype(np.uint8)
    volume = volume_of(vol, depth)
    plain = volume.labelComponents(connectivity)
    coords = all_coordinates(S)
    want_at, want_rec = plain.at(coords), plain.components()
    outside = np.array([[-1, 0, 0], [S, 3, 3], [2, 2, 1 << 20], [-(1 << 31), 0, 0]], np.int32)
    on_empty = np.argwhere(vol == 0)[::997][:9].astype(np.int32)
    for sites, r in ((outside, None), (outside, 4), (on_empty, 0)):
        labels = volume.fracture(sites, connectivity, False, r)
        assert labels.at(coords).tobytes() == want_at.tobytes() and labels.components().tobytes() == want_rec.tobytes()
        assert (labels.pieceSites() == NONE).all() and labels.count == plain.count
        labels.close()
    # one site, unlimited: the same pieces, every one in cell 0
    labels = volume.fracture([[5, 6, 7]], connectivity)
    assert labels.at(coords).tobytes() == want_at.tobytes() and labels.components().tobytes() == want_rec.tobytes()
    assert (labels.pieceSites() == 0).all()
    assert int(labels.components()["voxels"].sum()) == int(vol.sum())
    labels.close()
    plain.close()
    volume.close()


def test_a_box_split_by_two_sites(built):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 5, 32
    box = vrc.VoxelVolume(depth)
    box.fillBoxes([[0, 0, 0, S, S, S]])
    whole = box.labelComponents(6)
    want = whole.moments()
    whole.close()
    labels = box.fracture([[9, 20, 4], [22, 11, 27]])
    assert labels.count == 2 and sorted(labels.pieceSites().tolist()) == [0, 1]
    mo = labels.moments()
    assert int(mo["voxels"].sum()) == S ** 3 == int(want["voxels"][0])
    assert np.array_equal(mo["s1"].sum(axis=0), want["s1"][0]) and np.array_equal(mo["s2"].sum(axis=0), want["s2"][0])
    one = labels.select([1, 0])
    assert 0 < one.solidCount() < S ** 3
    labels.select([0, 1], one, vrc.capi.VRC_COPY_OR)
    assert np.array_equal(one.download(), box.download())
    for v in (one, labels, box):
        v.close()


# ---- memory kinds, windows --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def broken():
    """a 32^3 medium, 40 sites and the model's labelling of it, shared and left unchanged"""
    rng = np.random.default_rng(5150)
    vol = (rng.random((32, 32, 32)) < 0.5).astype(np.uint8)
    sites = random_sites(rng, 32, 40)
    ids, rec, ps = model.label(vol, sites, 6, False, 81)
    assert len(rec) > 100 and (ps == NONE).any() and (ps != NONE).any()
    return vol, sites, ids, rec, ps


def test_device_sites_windows_and_refusal(built, broken):
    import torch
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    vol, sites, ids, rec, ps = broken
    volume = volume_of(vol, 5)
    host = volume.fracture(sites, 6, False, 9)
    check_labels(host, ids, rec, ps, "host sites")
    t_sites = torch.from_numpy(sites).cuda()
    torch.cuda.synchronize()
    dev = volume.fractureDevice(len(sites), t_sites.data_ptr(), 6, False, 9)
    check_labels(dev, ids, rec, ps, "device sites")
    dev.close()
    Cn = host.count
    for first, capacity in [(0, 10), (0, 1), (Cn // 2 - 5, 10), (Cn - 3, 10), (Cn - 1, 1), (Cn, 4), (Cn + 5, 4), (0, Cn), (0, Cn + 9), (2 ** 40, 3)]:
        out = np.full(capacity + 3, 0xABABABAB, np.uint32)
        assert L.vrc_fracture_piece_sites(host._h, first, capacity, vrc.capi.ptr(out), vrc.capi.VRC_MEM_HOST, None) == 0
        k = max(0, min(capacity, Cn - first))
        assert np.array_equal(out[:k], ps[first:first + k]) and (out[k:] == 0xABABABAB).all(), (first, capacity)
        assert np.array_equal(host.pieceSites(first, capacity), ps[first:first + k])
    assert L.vrc_fracture_piece_sites(host._h, 0, 0, None, vrc.capi.VRC_MEM_HOST, None) == 0              # capacity 0, no buffer
    t_out = torch.full((Cn + 2,), 0x5A5A5A5A, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        host.pieceSitesDevice(7, Cn, t_out.data_ptr(), stream)                                           # a window that runs past the end
    got = t_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:Cn - 7], ps[7:]) and (got[Cn - 7:] == 0x5A5A5A5A).all()
    host.close()
    plain = volume.labelComponents(6)
    with pytest.raises(vrc.VrcError, match="vrc_fracture_piece_sites: not fracture labels"):
        plain.pieceSites()
    assert L.vrc_fracture_piece_sites(plain._h, 0, 0, None, vrc.capi.VRC_MEM_HOST, None) == -1
    plain.close()
    volume.close()


# ---- the snapshot -----------------------------------------------------------------------------------------------

def test_snapshot_order_and_bytes(built, broken):
    import torch
    vol, sites, ids, rec, ps = broken
    S = 32
    volume = volume_of(vol, 5)
    scratch = volume.editScratchBytes()
    plain = volume.labelComponents(6)
    labels = volume.fracture(sites, 6, False, 9)
    again = volume.fracture(sites, 6, False, 9)
    coords = all_coordinates(S)
    assert labels.at(coords).tobytes() == again.at(coords).tobytes() and labels.components().tobytes() == again.components().tobytes()
    assert labels.pieceSites().tobytes() == again.pieceSites().tobytes()
    again.close()
    assert volume.editScratchBytes() == scratch
    assert labels.bytes() == 4 * S ** 3 + 48 * labels.count + 4 * labels.count and plain.bytes() == 4 * S ** 3 + 48 * plain.count
    plain.close()
    # a device-memory edit on a stream immediately before the call is seen
    extra = np.ascontiguousarray(np.argwhere(vol == 0)[::3], np.uint32)          # argwhere is a transposed array: C order for the device
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        volume.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
        later = volume.fracture(sites, 6, False, 9)
    vol2 = vol.copy()
    vol2[tuple(extra.astype(np.int64).T)] = 1
    assert np.array_equal(volume.download(), vol2)
    ids2, rec2, ps2 = model.label(vol2, sites, 6, False, 81)
    check_labels(later, ids2, rec2, ps2, "behind a device edit")
    later.close()
    check_labels(labels, ids, rec, ps, "after edits of the medium")
    volume.close()
    check_labels(labels, ids, rec, ps, "after the medium is gone")
    labels.close()


# ---- beyond LDS -------------------------------------------------------------------------------------------------

def test_cells_at_256(built):
    """256^3 is the smallest size at which the envelope stacks leave LDS for device memory, and a column is four chunks of a
    wave.  12 sites, two of them duplicated and one outside; the cell of all 2^24 voxels against the model's brute force."""
    S = 256
    rng = np.random.default_rng(256)
    sites = rng.integers(0, S, (12, 3)).astype(np.int32)
    sites[7] = sites[2]
    sites[9] = (S, 5, 5)
    sites[4] = (sites[3][0], sites[3][1], (sites[3][2] + 100) % S)         # two in one column
    for r in (None, 90):
        want = model.cells(S, sites, NONE if r is None else r * r)
        got = device_cells(S, sites, r)
        assert np.array_equal(got, want), (r, np.argwhere(got != want)[:4].tolist())


# ---- shatter ----------------------------------------------------------------------------------------------------

def test_shatter_the_terrain(built, heights, textures):
    """The chain a game runs at 128^3: sites scattered round a point on the terrain's underside surface (the terrain is solid
    for y in [S/2 + 1, S/2 + lim) and the space towards -y below it is empty), the ground within 12 voxels of them broken into
    shards; eight of the twelve fall 65 cells towards -y to the volume's face, four stay wedged.  The result is the model
    chain's, the committed scene the host builder's, and a 64 x 64 frame of it the oracle's."""
    import cpuvoxelraycaster_amd as vrc
    import test_gpu_volume as V
    depth, S, W, Hh = 7, 128, 64, 64
    terrain = V.terrain_volume(heights, depth)
    x, z = 61, 40
    low = int(np.flatnonzero(terrain[x, :, z]).min())
    sites = vrc.scatter_sites((x, low, z), 7, 14, 3)
    down, r = vrc.capi.VRC_FACE_YN, 12
    # the model chain
    ids, rec, ps = model.label(terrain, sites, 6, False, r * r)
    shard = ps != NONE
    assert shard.sum() >= 5 and (~shard).sum() >= 1
    rest = terrain & (1 - components_model.select(ids, shard))
    D = fall_model.drops(ids, rest, down)
    want = fall_model.place(ids, fall_model.offsets_of(D, down), rest, keep=shard)
    assert (D[~shard] == 0).all() and int(want.sum()) == int(terrain.sum())
    assert (D > 0).sum() >= 5 and (D[shard] == 0).sum() >= 2 and int(D.max()) == S // 2 + 1

    scene = vrc.LSVO.fromTerrain(heights, depth, textures=textures)
    volume = vrc.VoxelVolume.fromScene(scene)
    before = volume.solidCount()
    stats, labels = volume.shatter(sites, r, down)
    check_labels(labels, ids, rec, ps, "shatter")
    labels.close()
    assert fall_model.stats_tuple(stats) == fall_model.stats(ids, D)
    assert volume.solidCount() == before
    got = volume.download()
    assert np.array_equal(got, want)
    far = np.ones((S, S, S), bool)
    far[max(0, x - 24):x + 24, :, max(0, z - 24):z + 24] = False
    assert np.array_equal(got[far], terrain[far])                           # nothing of the far world moved
    after = volume.commit()
    nodes = after.downloadNodes()
    assert V.same(nodes, vrc.build_volume_lsvo(want, depth))
    cam, light = vrc.reference_camera(depth, pitch=-0.5), vrc.reference_light(depth)
    rc = vrc.RayCaster(after, (W, Hh))
    rc.setLightPosition(light)
    rc.use_gi = rc.use_samples = True
    rc.shadow_samples = 1
    rc.renderFrame(cam, spp=1)
    want_acc, frame_stats = V.oracle_frame(nodes, depth, textures, cam, light, W, Hh, 1)
    assert np.array_equal(rc.readAccum(), want_acc) and V.stats_tuple(rc.stats()) == frame_stats
    for v in (rc, after, volume, scene):
        v.close()
