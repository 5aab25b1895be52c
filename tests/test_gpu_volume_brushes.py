"""Brushes, region copies and queries of the editable volume on the GPU (vrc_volume_fill_spheres[_at_hits],
vrc_volume_copy_region, vrc_volume_clone, vrc_volume_get_voxels, vrc_volume_count_boxes).  Every expected value comes from
a numpy occupancy array edited with numpy, the oracle's compileSVO / the host builder for the committed LNode[], the
oracle's castRay for hits and the host function vrc_hit_to_voxel; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import raygen
from volume_support import Stream, committed, expected_nodes, same, terrain_volume

pytestmark = pytest.mark.gpu

LIMIT = 1 << 20


def check_volume(volume, vol, depth, what, commit=True):
    assert np.array_equal(volume.download(), vol), what
    assert volume.solidCount() == int(vol.sum(dtype=np.int64)), what
    if commit:
        assert same(committed(volume), expected_nodes(vol, depth)), what


def random_volume(depth, density, seed):
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    vol = (np.random.default_rng(seed).random((S, S, S)) < density).astype(np.uint8)
    scene = vrc.LSVO.fromVolume(vol, depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    scene.close()
    return vol, volume


# ---- 1. spheres ------------------------------------------------------------------------------------------------

def numpy_spheres(vol, spheres, value):
    """(dx*dx + dy*dy + dz*dz <= r*r) on an integer ogrid, restricted to the sphere's clipped bounding box"""
    S = vol.shape[0]
    for cx, cy, cz, r in np.asarray(spheres, np.int64):
        if r < 0 or r > LIMIT or max(abs(cx), abs(cy), abs(cz)) > LIMIT:
            continue
        lo = [max(0, c - r) for c in (cx, cy, cz)]
        hi = [min(S, c + r + 1) for c in (cx, cy, cz)]
        if any(l >= h for l, h in zip(lo, hi)):
            continue
        x, y, z = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        inside = (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r
        vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][inside] = value


def sphere_groups(S):
    m, e = S // 2, S - 1
    radii = [0, 1, 2, 7, S // 4, S, 2 * S]
    faces = [(0, m, m), (e, m, m), (m, 0, m), (m, e, m), (m, m, 0), (m, m, e)]
    corners = [(x, y, z) for x in (0, e) for y in (0, e) for z in (0, e)]
    return [
        ("radii at an inside centre", True, [(m + 1, m - 2, m + 3, r) for r in radii[:5]]),
        ("carve at odd centres", False, [(m - 3, m + 1, m - 1, 7), (5, 6, 7, 2), (m, m, m, 0)]),
        ("faces", True, [c + (r,) for c, r in zip(faces, [0, 1, 2, 7, 7, S // 4])]),
        ("corners", False, [c + (r,) for c, r in zip(corners, [0, 1, 2, 7, 7, 2, 1, S // 4])]),
        ("outside by less than r", True, [(-3, m, m, 7), (m, S + 4, m, 7), (m, m, -1, 2), (S, S, S, 2), (-5, -5, -5, 9)]),
        ("outside by more than r", True, [(-8, m, m, 7), (m, S + 8, m, 7), (m, m, -3, 2), (-100000, 3, 3, 50), (S + 2, 1, 1, 1)]),
        ("negative centres, negative radius", False, [(-1, -1, -1, 2), (-2, 3, -4, 7), (m, m, m, -1), (3, 3, 3, -LIMIT)]),
        ("radius S", False, [(m, m, m, S)]),                                    # everything
        ("radius 2S from outside", True, [(-S, m, m, 2 * S)]),
        ("bounds of a dropped item", False, [(LIMIT + 1, m, m, LIMIT), (m, -LIMIT - 1, m, LIMIT), (m, m, m, LIMIT + 1),
                                             (-0x80000000, 0x7fffffff, 0, 0x7fffffff)]),                # all dropped
        ("the largest centre kept", False, [(m, m, LIMIT, LIMIT - m)]),          # reaches z = m from 2^20 away
        ("the largest radius kept", False, [(m, m, m, LIMIT)]),                  # next to the dropped 2^20 + 1: clears everything
        ("overlapping and duplicate", True, [(m, m, m, 7), (m + 3, m, m, 7), (m, m, m, 7), (m, m + 5, m - 2, 2), (m, m, m, 7)]),
        ("carve inside what was set", False, [(m + 1, m, m, 2), (m + 1, m, m, 2)]),
    ]


@pytest.mark.parametrize("depth", [5, 8])
def test_fill_spheres(built, depth):
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    vol, volume = random_volume(depth, 0.05, depth)
    device = volume.clone()
    with Stream() as stream:
        for i, (what, solid, spheres) in enumerate(sphere_groups(S)):
            arr = np.array(spheres, np.int64).astype(np.int32)
            volume.fillSpheres(arr, solid)
            t = torch.from_numpy(arr.copy()).cuda()
            torch.cuda.synchronize()
            device.fillSpheresDevice(len(arr), t.data_ptr(), solid, stream)
            numpy_spheres(vol, spheres, 1 if solid else 0)
            check_volume(volume, vol, depth, (depth, what))
            assert np.array_equal(device.download(), vol), (depth, what)       # download waits for the stream's edit
    rng = np.random.default_rng(100 + depth)
    many = np.concatenate([rng.integers(-4, S + 4, (4096, 3)), rng.integers(-1, 5, (4096, 1))], axis=1).astype(np.int32)
    for solid in (True, False):
        batch = many[:2048] if solid else many[2048:]
        volume.fillSpheres(batch, solid)
        numpy_spheres(vol, batch, 1 if solid else 0)
    check_volume(volume, vol, depth, (depth, "4096 random small spheres"))
    volume.fillSpheres(many, True)                                             # all 4096 in one batch
    numpy_spheres(vol, many, 1)
    check_volume(volume, vol, depth, (depth, "one batch of 4096"))


# ---- 2. brush at ray hits ----------------------------------------------------------------------------------------

def ball_offsets(r):
    g = np.mgrid[-r:r + 1, -r:r + 1, -r:r + 1].reshape(3, -1).T
    return g[(g * g).sum(1) <= r * r]


def numpy_spheres_at(vol, centres, r, value):
    """the same predicate for many centres of one radius: every offset of the ball applied to every centre"""
    S = vol.shape[0]
    centres = np.asarray(centres, np.int64).reshape(-1, 3)
    for off in ball_offsets(r):
        p = centres + off
        p = p[np.all((p >= 0) & (p < S), axis=1)]
        vol[p[:, 0], p[:, 1], p[:, 2]] = value


def host_centres(depth, records):
    """The host function vrc_hit_to_voxel per record (what vrc.hit_to_voxel calls): (dig centres, build centres).  The
    records it refuses are skipped, and a build needs a neighbour."""
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    records = np.ascontiguousarray(records, vrc.HIT_DTYPE)
    voxel, neighbour, has = np.zeros(3, np.uint32), np.zeros(3, np.uint32), C.c_int()
    pv, pn, ph = vrc.capi.ptr(voxel), vrc.capi.ptr(neighbour), C.byref(has)
    dig, build = [], []
    for i in range(len(records)):
        if L.vrc_hit_to_voxel(depth, C.c_void_p(records.ctypes.data + 48 * i), pv, pn, ph) != 0:
            continue
        dig.append(tuple(voxel))
        if has.value:
            build.append(tuple(neighbour))
    return np.array(dig, np.int64).reshape(-1, 3), np.array(build, np.int64).reshape(-1, 3)


def test_brush_at_hits_of_a_device_batch(built, heights):
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth = 9
    nodes = vrc.build_terrain_lsvo(heights, depth)
    org, d = raygen.camera_rays(depth, 960, 540, 0.0)
    n = len(org)
    ref = O.cast_rays(nodes, depth, org, d, threads=8)
    kind = ref["hit"] & 0xff
    multi = ((ref["normal"] != 0).sum(1) > 1) & (kind == 1)
    print(f"oracle records: {int((kind == 1).sum())} unit-voxel hits, {int((kind == 0).sum())} misses, {int(multi.sum())} multi-axis normals of {n}")
    assert (kind == 1).sum() >= 0.3 * n and (kind == 0).sum() >= 0.3 * n and multi.sum() >= 1
    ref_lod = O.cast_rays(nodes, depth, org, d, coef=0.5, threads=8)
    assert ((ref_lod["hit"] & 0xff) == 2).sum() > 0
    unit = ref[kind == 1]
    dig_at, build_at = host_centres(depth, unit)
    assert len(host_centres(depth, ref[kind != 1][::97])[0]) == 0          # the host function refuses a miss
    lod_dig_at, _ = host_centres(depth, ref_lod[(ref_lod["hit"] & 0xff) == 1])
    assert len(dig_at) == len(unit) and 0 < len(build_at) < len(unit)

    scene = vrc.LSVO(nodes, depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    vol = terrain_volume(heights, depth)
    t_org, t_dir = torch.from_numpy(org).cuda(), torch.from_numpy(d).cuda()
    t_coef = torch.full((n,), 0.5, dtype=torch.float32).cuda()
    t_hits = torch.zeros(n * 12, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        for solid, radius in ((False, 0), (True, 0), (False, 3), (True, 2)):
            scene.castRaysDevice(n, t_org.data_ptr(), t_dir.data_ptr(), t_hits.data_ptr(), stream=stream)
            volume.fillSpheresAtHitsDevice(n, t_hits.data_ptr(), radius, solid, stream)      # nothing between the two calls
            numpy_spheres_at(vol, build_at if solid else dig_at, radius, 1 if solid else 0)
            check_volume(volume, vol, depth, ("at hits", solid, radius), commit=(solid, radius) in ((False, 3), (True, 2)))
        # the LOD batch: its cut-off records (kind 2) are skipped, its unit-voxel records (if any) dig
        scene.castRaysDevice(n, t_org.data_ptr(), t_dir.data_ptr(), t_hits.data_ptr(), coef_ptr=t_coef.data_ptr(), stream=stream)
        volume.fillSpheresAtHitsDevice(n, t_hits.data_ptr(), 3, False, stream)
        numpy_spheres_at(vol, lod_dig_at, 3, 0)
        check_volume(volume, vol, depth, "LOD batch", commit=False)
    # the host-memory form on the oracle's records gives the same volume
    other = vrc.VoxelVolume.fromScene(scene)
    other.fillSpheresAtHits(ref, 0, False)
    other.fillSpheresAtHits(ref, 0, True)
    other.fillSpheresAtHits(ref, 3, False)
    other.fillSpheresAtHits(ref, 2, True)
    other.fillSpheresAtHits(ref_lod, 3, False)
    assert np.array_equal(other.download(), vol)


def test_host_edits_behind_a_pending_device_brush(built):
    """The device-memory brush leaves its centres in the volume's staging block, in flight on the caller's stream.  Host-memory
    edits issued right behind it -- on the NULL stream and on a second created stream, neither of which waits for the first
    by itself -- go through the same block and must not reach it before the brush has read its centres."""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth = 8
    S = 1 << depth
    rng = np.random.default_rng(8)
    n = 400000
    hits = np.zeros(n, vrc.HIT_DTYPE)
    hits["hit"] = 1
    hits["position"] = (1.0 + rng.random((n, 3)) * 0.999).astype(np.float32)
    hits["normal"][:, 1] = -2
    dig_at, build_at = host_centres(depth, hits[:1000])
    assert len(build_at) > 900
    g = np.float32(S)
    cells = (S - 1 - np.floor((hits["position"] - np.float32(1.0)) * g)).astype(np.int64)     # vrc_hit_to_voxel, checked on the first 1000
    assert np.array_equal(cells[:1000], dig_at)
    t_hits = torch.from_numpy(hits.view(np.int32).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    vol, volume = random_volume(depth, 0.5, 81)
    few = np.array([(1, 2, 3), (200, 100, 50)], np.uint32)                 # 24 bytes: fits the block the brush is using
    box = np.array([(0, 0, 0, 9, 9, 9)], np.uint32)
    sphere = np.array([(S - 1, S - 1, S - 1, 6)], np.int32)
    with Stream() as a, Stream() as b:
        for round_ in range(3):
            volume.fillSpheresAtHitsDevice(n, t_hits.data_ptr(), 2, False, a)
            volume.setVoxels(few, True)                                    # host form, NULL stream
            numpy_spheres_at(vol, cells, 2, 0)
            vol[few[:, 0], few[:, 1], few[:, 2]] = 1
            volume.fillSpheresAtHitsDevice(n, t_hits.data_ptr(), 1, True, a)
            assert int(volume.getVoxels(few).sum()) >= 0                   # a query on the NULL stream in between
            volume.fillSpheresAtHitsDevice(n, t_hits.data_ptr(), 0, False, b)      # a second stream reuses the block
            L = vrc.capi.load()
            vrc.capi.check(L.vrc_volume_fill_boxes(volume._h, 1, vrc.capi.ptr(box), 0, vrc.capi.VRC_MEM_HOST, b))
            volume.fillSpheres(sphere, round_ % 2 == 0)
            inside = cells.copy()
            inside[:, 1] += 1                                              # the neighbour of normal (0, -2, 0)
            numpy_spheres_at(vol, inside[inside[:, 1] < S], 1, 1)
            numpy_spheres_at(vol, cells, 0, 0)
            vol[0:9, 0:9, 0:9] = 0
            numpy_spheres(vol, sphere, 1 if round_ % 2 == 0 else 0)
            check_volume(volume, vol, depth, ("behind a pending brush", round_), commit=round_ == 2)


def test_brush_at_hand_made_records(built):
    import cpuvoxelraycaster_amd as vrc
    depth = 5
    S = 1 << depth
    rec = np.zeros(12, vrc.HIT_DTYPE)
    rec["hit"] = 1
    rec["position"] = (1.5, 1.25, 1.75)
    rec["normal"] = (0, -2, 0)
    rec["position"][1] = (np.nan, 1.5, 1.5)
    rec["position"][2] = (1.0, 1.0, 1.0)                 # exactly 1.0: the last voxel of the reflected volume
    rec["position"][3] = (2.0, 1.5, 1.5)                 # exactly 2.0: outside
    rec["normal"][4] = (0, 0, 0)                         # no neighbour: the ray started inside
    rec["position"][5] = (1.5, 1.5, 1.999)
    rec["normal"][5] = (0, 0, 4)                         # neighbour z = -1: outside the volume
    rec["normal"][6] = (1, 2, 0)                         # multi-axis
    rec["hit"][7] = 0                                    # miss
    rec["hit"][8] = 2 | (3 << 8)                         # LOD cut-off
    rec["position"][9] = (0.5, 1.5, 1.5)
    rec["position"][10] = (1.5, np.inf, 1.5)
    rec["position"][11] = (np.nextafter(np.float32(2.0), np.float32(0)), 1.5, 1.5)   # the first voxel
    for solid in (False, True):
        for radius in (0, 2):
            vol, volume = random_volume(depth, 0.3, 7)
            volume.fillSpheresAtHits(rec, radius, solid)
            at = host_centres(depth, rec)[1 if solid else 0]
            assert len(at) == (2 if solid else 6)           # dig: records 0, 2, 4, 5, 6, 11; build: 0 and 11
            numpy_spheres_at(vol, at, radius, 1 if solid else 0)
            check_volume(volume, vol, depth, ("hand-made", solid, radius))
    corner_dig, corner_build = host_centres(depth, rec[2:3])                 # position 1.0: the corner voxel, its neighbour outside
    assert corner_dig.tolist() == [[S - 1, S - 1, S - 1]] and len(corner_build) == 0


# ---- 3. the dig is seen by the next ray ----------------------------------------------------------------------------

def autofocus_ray(depth, cam):
    S = np.float32(1 << depth)
    org = (np.array(tuple(cam.position), np.float32) / S + np.float32(1.0)).astype(np.float32)
    rot = np.array(tuple(cam.rot), np.float32)
    return org, np.array([rot[2], rot[5], rot[8]], np.float32)


def test_dig_is_seen_by_the_next_ray(built, heights):
    import cpuvoxelraycaster_amd as vrc
    depth = 8
    vol = terrain_volume(heights, depth)
    scene = vrc.LSVO.fromTerrain(heights, depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    org, d = autofocus_ray(depth, vrc.reference_camera(depth, pitch=-0.5))
    first = scene.castRay(org, d)
    voxel, _ = vrc.hit_to_voxel(depth, first)
    assert vol[voxel] == 1
    volume.fillSpheresAtHits(np.array([first]), 3, False)
    numpy_spheres(vol, [voxel + (3,)], 0)
    dug = volume.commit()
    want_nodes = expected_nodes(vol, depth)
    assert same(dug.downloadNodes(), want_nodes)
    second = dug.castRay(org, d)
    assert second.tobytes() == O.cast_rays(want_nodes, depth, org[None], d[None])[0].tobytes()
    assert (second["hit"] & 0xff) == 1 and second["distance"] > first["distance"]


# ---- 4. region copy --------------------------------------------------------------------------------------------------

def numpy_copy(dst, src, src_lo, size, dst_lo, op):
    Sd, Ss = dst.shape[0], src.shape[0]
    lo, hi = [], []
    for a in range(3):
        d0 = max(0, -int(dst_lo[a]))
        d1 = min(int(size[a]), Ss - int(src_lo[a]), Sd - int(dst_lo[a]))
        if d0 >= d1:
            return
        lo.append(d0)
        hi.append(d1)
    s = src[tuple(slice(int(src_lo[a]) + lo[a], int(src_lo[a]) + hi[a]) for a in range(3))]
    where = tuple(slice(int(dst_lo[a]) + lo[a], int(dst_lo[a]) + hi[a]) for a in range(3))
    if op == 0:
        dst[where] = s
    elif op == 1:
        dst[where] |= s
    else:
        dst[where] &= 1 - s


def copy_cases(Ss, Sd, rng):
    cases = []
    for rz in range(8):                                  # dst_lo - src_lo mod 8 on z: all residues; mod 2 on x and y: all four
        for px in range(2):
            for py in range(2):
                size = [1, 2, 3, 8, 9, Ss][(rz + px + 2 * py) % 6]
                src_lo = [int(v) for v in rng.integers(0, max(1, Ss - size + 1), 3)]
                base = [int(v) for v in rng.integers(0, max(1, (Sd - size) // 8), 3) * 8]
                dst_lo = [src_lo[0] % 8 + base[0] + px, src_lo[1] % 8 + base[1] + py, src_lo[2] % 8 + base[2] + rz]
                cases.append((src_lo, [size] * 3, dst_lo))
    q = Ss // 4
    cases += [
        ([Ss - 5, q, q], [9, 9, 9], [8, 9, 11]),                               # clipped by src
        ([q, q, q], [9, 9, 9], [Sd - 4, 3, Sd - 1]),                           # clipped by dst
        ([Ss - 3, q, 0], [9, Ss, 9], [Sd - 7, -5, -3]),                        # by both, negative dst_lo
        ([0, 0, 0], [Ss, Ss, Ss], [-3, -1, -7]),
        ([0, 0, 0], [Ss + 9, 0xffffffff, Ss], [1, 2, 3]),                      # size beyond everything
        ([Ss, 0, 0], [4, 4, 4], [0, 0, 0]), ([0, 0, 0], [4, 4, 4], [Sd, 0, 0]), ([0, 0, 0], [4, 4, 4], [0, -4, 0]),   # wholly outside
        ([1, 1, 1], [0, 4, 4], [0, 0, 0]),                                     # empty
        ([1, 2, 3], [5, 1, 2], [Sd - 5, Sd - 1, Sd - 2]),                      # the last voxels
    ]
    return cases


@pytest.mark.parametrize("src_depth,dst_depth", [(5, 8), (8, 8), (3, 2), (2, 3)])
def test_copy_region(built, src_depth, dst_depth):
    import cpuvoxelraycaster_amd as vrc
    Ss, Sd = 1 << src_depth, 1 << dst_depth
    rng = np.random.default_rng(src_depth * 10 + dst_depth)
    svol, src = random_volume(src_depth, 0.3, 40 + src_depth)
    dvol, dst = random_volume(dst_depth, 0.3, 50 + dst_depth)
    if min(Ss, Sd) >= 32:
        cases = copy_cases(Ss, Sd, rng)
        assert {((c[2][2] - c[0][2]) % 8, (c[2][0] - c[0][0]) % 2, (c[2][1] - c[0][1]) % 2) for c in cases[:32]} == \
            {(z, x, y) for z in range(8) for x in range(2) for y in range(2)}
    else:                                                # tiny volumes: two brick rows share a word at 4^3
        cases = [([int(v) for v in rng.integers(0, Ss, 3)], [int(v) for v in rng.integers(1, Ss + 2, 3)],
                  [int(v) for v in rng.integers(-2, Sd, 3)]) for _ in range(40)]
    for i, (src_lo, size, dst_lo) in enumerate(cases):
        op = i % 3
        dst.copyRegion(src, src_lo, size, dst_lo, op)
        numpy_copy(dvol, svol, src_lo, size, dst_lo, op)
        if i % 8 == 7 or i >= 32 or Sd < 32:
            assert np.array_equal(dst.download(), dvol), (i, src_lo, size, dst_lo, op)   # the whole volume: nothing outside the region moved
    check_volume(dst, dvol, dst_depth, "after the copies")
    for op in (0, 1, 2):                                 # the three ops once more on one large odd-offset region
        size = [Ss - 2, Ss, max(1, Ss - 5)]
        dst.copyRegion(src, [1, 0, 3], size, [2 + op, 1, 6 - op], op)
        numpy_copy(dvol, svol, [1, 0, 3], size, [2 + op, 1, 6 - op], op)
        check_volume(dst, dvol, dst_depth, ("op", op), commit=op == 2)
    assert np.array_equal(src.download(), svol)          # the source is only read


def test_copy_region_behind_device_edits_and_refusals(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    svol, src = random_volume(5, 0.3, 1)
    dvol, dst = random_volume(8, 0.3, 2)
    spheres = np.array([(16, 16, 16, 9), (3, 30, 8, 5)], np.int32)
    boxes = np.array([(0, 0, 0, 32, 4, 32)], np.uint32)
    t_s, t_b = torch.from_numpy(spheres).cuda(), torch.from_numpy(boxes.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        src.fillSpheresDevice(2, t_s.data_ptr(), True, stream)
        src.fillBoxesDevice(1, t_b.data_ptr(), False, stream)
        dst.copyRegion(src, [0, 0, 0], [32, 32, 32], [101, 77, 203], vrc.capi.VRC_COPY_REPLACE, stream)
        numpy_spheres(svol, spheres, 1)
        svol[0:32, 0:4, 0:32] = 0
        numpy_copy(dvol, svol, [0, 0, 0], [32, 32, 32], [101, 77, 203], 0)
        check_volume(dst, dvol, 8, "copy behind edits of src")     # download / count / commit wait for dst's recorded edit
    z3, one3 = np.zeros(3, np.uint32), np.ones(3, np.uint32)
    i3 = np.zeros(3, np.int32)
    p = vrc.capi.ptr
    assert L.vrc_volume_copy_region(dst._h, dst._h, p(z3), p(one3), p(i3), 0, None) == -1
    assert b"same volume" in L.vrc_last_error()
    for op in (-1, 3):
        assert L.vrc_volume_copy_region(dst._h, src._h, p(z3), p(one3), p(i3), op, None) == -1
    assert L.vrc_volume_copy_region(dst._h, src._h, None, p(one3), p(i3), 0, None) == -1
    assert L.vrc_volume_copy_region(dst._h, src._h, p(z3), None, p(i3), 0, None) == -1
    assert L.vrc_volume_copy_region(dst._h, src._h, p(z3), p(one3), None, 0, None) == -1
    assert np.array_equal(dst.download(), dvol)


def test_argument_checks_on_a_live_volume(built):
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    p = vrc.capi.ptr
    vol, volume = random_volume(4, 0.3, 3)
    v = volume._h
    buf = np.zeros(64, np.uint32)
    hits = np.zeros(2, vrc.HIT_DTYPE)
    out8, out64 = np.zeros(8, np.uint8), np.zeros(8, np.uint64)
    for mem in (0, 1):                                   # n == 0 is VRC_OK, whatever the buffers
        assert L.vrc_volume_fill_spheres(v, 0, None, 1, mem, None) == 0
        assert L.vrc_volume_fill_spheres_at_hits(v, 0, None, 1, 1, mem, None) == 0
        assert L.vrc_volume_get_voxels(v, 0, None, None, mem, None) == 0
        assert L.vrc_volume_count_boxes(v, 0, None, None, mem, None) == 0
    assert L.vrc_volume_fill_spheres(v, 2, None, 1, 0, None) == -1
    assert L.vrc_volume_fill_spheres(v, 2, p(buf), 1, 2, None) == -1
    assert L.vrc_volume_fill_spheres_at_hits(v, 2, None, 1, 1, 0, None) == -1
    assert L.vrc_volume_fill_spheres_at_hits(v, 2, p(hits), 1, 1, 7, None) == -1
    assert L.vrc_volume_fill_spheres_at_hits(v, 2, p(hits), -1, 1, 0, None) == -1
    assert L.vrc_volume_fill_spheres_at_hits(v, 2, p(hits), LIMIT + 1, 1, 0, None) == -1
    assert L.vrc_volume_fill_spheres_at_hits(v, 2, p(hits), LIMIT, 0, 0, None) == 0      # two misses: nothing happens
    assert L.vrc_volume_get_voxels(v, 2, None, p(out8), 0, None) == -1
    assert L.vrc_volume_get_voxels(v, 2, p(buf), None, 0, None) == -1
    assert L.vrc_volume_get_voxels(v, 2, p(buf), p(out8), -1, None) == -1
    assert L.vrc_volume_count_boxes(v, 2, None, p(out64), 0, None) == -1
    assert L.vrc_volume_count_boxes(v, 2, p(buf), None, 0, None) == -1
    assert L.vrc_volume_count_boxes(v, 2, p(buf), p(out64), 5, None) == -1
    assert np.array_equal(volume.download(), vol)


# ---- 5. clone --------------------------------------------------------------------------------------------------------

def test_clone(built, heights, textures):
    import cpuvoxelraycaster_amd as vrc
    depth, W, H = 8, 64, 36
    vol = terrain_volume(heights, depth)
    scene = vrc.LSVO.fromTerrain(heights, depth, textures=textures)
    volume = vrc.VoxelVolume.fromScene(scene)
    volume.fillSpheres([(128, 80, 128, 20)], False)
    numpy_spheres(vol, [(128, 80, 128, 20)], 0)
    snapshot = volume.clone()
    assert snapshot.depth == depth and np.array_equal(snapshot.download(), vol)
    assert same(committed(snapshot), committed(volume)) and same(committed(snapshot), expected_nodes(vol, depth))

    def frame(svo):
        rc = vrc.RayCaster(svo, (W, H))
        rc.setLightPosition(vrc.reference_light(depth))
        rc.use_gi = rc.use_samples = True
        rc.renderFrame(vrc.reference_camera(depth, pitch=-0.5), spp=2)
        rc.samples_to_image()
        return rc.readImage()

    a, b = volume.commit(), snapshot.commit()            # the albedo tables travel: the same textured frame
    white = vrc.VoxelVolume(depth)
    white.copyRegion(volume, [0, 0, 0], [256, 256, 256], [0, 0, 0])
    c = white.commit()
    img = frame(a)
    assert np.array_equal(frame(b), img)
    assert same(c.downloadNodes(), a.downloadNodes()) and not np.array_equal(frame(c), img)   # same voxels, white tables
    # editing either leaves the other as it was
    edited = vol.copy()
    volume.fillSpheres([(100, 100, 100, 9)], True)
    numpy_spheres(edited, [(100, 100, 100, 9)], 1)
    assert np.array_equal(volume.download(), edited) and np.array_equal(snapshot.download(), vol)
    snapshot.fillBoxes([(0, 0, 0, 256, 256, 8)], True)
    assert np.array_equal(volume.download(), edited)
    volume.close()                                       # and the clone outlives the original
    vol[:, :, 0:8] = 1
    check_volume(snapshot, vol, depth, "clone after the original is gone")


# ---- 6. queries ------------------------------------------------------------------------------------------------------

def box_cases(S):
    h = S // 2
    return [
        [(0, 0, 0, h, h, h)],
        [(h + 1, 3, 5, S - 1, h - 1, S - 3)],
        [(2, 2, 2, h - 1, h - 2, h - 3)],
        [(3, 0, 0, 4, S, S), (0, 5, 0, S, 6, S), (0, 0, 7, S, S, 8)],
        [(4, 4, 4, 4, 9, 9), (9, 9, 9, 3, 3, 3), (S, 0, 0, S + 4, 4, 4)],
        [(h - 3, h - 3, h - 3, S + 100, 0xffffffff, S)],
        [(1, 1, 1, h, h, h), (h - 4, h - 4, h - 4, h + 5, h + 5, h + 5), (h - 4, 1, h - 4, h + 5, h, h + 5)],
        [(0, 0, 0, S, S, 1), (0, 0, S - 1, S, S, S), (0, 0, 1, S, S, 3), (5, 6, 0, 6, 7, S)],
        [(0, 0, 0, S, S, S)],
        [(1, 1, 1, S - 1, S - 1, S - 1)],
    ]


@pytest.mark.parametrize("depth", [5, 8])
def test_queries(built, depth):
    import torch
    import cpuvoxelraycaster_amd as vrc
    S = 1 << depth
    vol, volume = random_volume(depth, 0.3, 60 + depth)
    rng = np.random.default_rng(depth)
    xyz = rng.integers(0, S + S // 4, (100000, 3)).astype(np.uint32)
    xyz[::1000] = (0xffffffff, 1, 1)
    inside = np.all(xyz < S, axis=1)
    assert 1000 < inside.sum() < len(xyz) - 1000
    want = np.zeros(len(xyz), np.uint8)
    want[inside] = vol[xyz[inside, 0], xyz[inside, 1], xyz[inside, 2]]
    assert np.array_equal(volume.getVoxels(xyz), want)
    boxes = np.array([b for case in box_cases(S) for b in case], np.uint64).astype(np.uint32)
    counts = []
    for x0, y0, z0, x1, y1, z1 in boxes.astype(np.int64):
        ok = x0 < x1 and y0 < y1 and z0 < z1
        counts.append(int(vol[x0:min(x1, S), y0:min(y1, S), z0:min(z1, S)].sum(dtype=np.int64)) if ok else 0)
    assert volume.countBoxes(boxes).tolist() == counts
    assert int(volume.countBoxes([(0, 0, 0, S, S, S)])[0]) == volume.solidCount() == int(vol.sum(dtype=np.int64))
    # device memory, on a created stream right behind an edit: the queries see it
    t_xyz, t_boxes = torch.from_numpy(xyz.view(np.int32)).cuda(), torch.from_numpy(boxes.view(np.int32)).cuda()
    t_out, t_counts = torch.full((len(xyz),), 7, dtype=torch.uint8).cuda(), torch.full((len(boxes),), -1, dtype=torch.int64).cuda()
    sphere = np.array([(S // 2, S // 2, S // 2, S // 3)], np.int32)
    t_sphere = torch.from_numpy(sphere).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        volume.fillSpheresDevice(1, t_sphere.data_ptr(), False, stream)
        volume.getVoxelsDevice(len(xyz), t_xyz.data_ptr(), t_out.data_ptr(), stream)
        volume.countBoxesDevice(len(boxes), t_boxes.data_ptr(), t_counts.data_ptr(), stream)
        vrc.capi.check(vrc.capi.load().vrc_stream_synchronize(0, stream))
    numpy_spheres(vol, sphere, 0)
    want[inside] = vol[xyz[inside, 0], xyz[inside, 1], xyz[inside, 2]]
    assert np.array_equal(t_out.cpu().numpy(), want)
    counts = []
    for x0, y0, z0, x1, y1, z1 in boxes.astype(np.int64):
        ok = x0 < x1 and y0 < y1 and z0 < z1
        counts.append(int(vol[x0:min(x1, S), y0:min(y1, S), z0:min(z1, S)].sum(dtype=np.int64)) if ok else 0)
    assert t_counts.cpu().numpy().tolist() == counts
    assert volume.getVoxels(xyz[:0]).shape == (0,) and volume.countBoxes(np.zeros((0, 6))).shape == (0,)


# ---- 7. no growth ----------------------------------------------------------------------------------------------------

def test_brush_copy_query_rounds_do_not_grow(built):
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth = 8
    S = 1 << depth
    _, volume = random_volume(depth, 0.1, 70)
    _, stamp = random_volume(5, 0.3, 71)
    rng = np.random.default_rng(72)
    hits = np.zeros(5000, vrc.HIT_DTYPE)
    hits["hit"] = 1
    hits["position"] = (1.0 + rng.random((5000, 3)) * 0.999).astype(np.float32)
    hits["normal"][:, 1] = -2
    spheres = np.concatenate([rng.integers(0, S, (5000, 3)), rng.integers(0, 6, (5000, 1))], axis=1).astype(np.int32)
    xyz = rng.integers(0, S, (20000, 3)).astype(np.uint32)
    boxes = np.array([(0, 0, 0, S, S, S)] * 100, np.uint32)
    used = {}
    for i in range(1, 201):
        volume.fillSpheres(spheres, i % 2 == 1)
        volume.fillSpheresAtHits(hits, 2, i % 2 == 0)
        volume.copyRegion(stamp, [0, 0, 0], [32, 32, 32], [i % 200, 3, (7 * i) % 200], i % 3)
        volume.getVoxels(xyz)
        counts = volume.countBoxes(boxes)
        if i in (1, 2, 199, 200):
            assert int(counts[0]) == volume.solidCount()
            torch.cuda.synchronize()
            free, total = torch.cuda.mem_get_info()
            used[i] = total - free
    print("device memory in use after round 1, 2, 199, 200:", used[1], used[2], used[199], used[200])
    assert used[199] <= used[1] and used[200] <= used[1]
