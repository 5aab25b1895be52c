"""Falling pieces on the GPU (vrc_fall_drops, vrc_fall_place; VoxelLabels.fall / place, VoxelVolume.dropLoose).  The
expected drops are the tick simulation of tests/fall_model.py (held against the rule taken literally in
tests/test_volume_fall_host.py), the expected ids the labelling model's, or the analytic answer where a test says so.  Every
comparison is exact: the offsets, the stats (all but `rounds`, which is bounded by 1 <= rounds <= C + 1) and every voxel of
the placed volume."""

import numpy as np
import pytest

import components_model
import fall_model as model
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu
NONE = model.NONE


def check_fall(debris, fixed, connectivity, direction, limit=0, device_memory=False, through_empty=False, ids=None, what=None):
    """labels `debris`, lets the pieces fall over `fixed` (None: NULL) and places them into a copy of it; offsets, stats and
    the placed volume against the model.  Returns (D, stats)."""
    import cpuvoxelraycaster_amd as vrc
    S = debris.shape[0]
    depth = S.bit_length() - 1
    if ids is None:
        ids = components_model.label(debris, connectivity, through_empty)[0]
    D = model.drops(ids, fixed, direction, limit)
    want = model.offsets_of(D, direction)
    base = np.zeros((S, S, S), np.uint8) if fixed is None else fixed
    medium = volume_of(debris, depth)
    labels = medium.labelComponents(connectivity, through_empty)
    medium.close()
    assert labels.count == len(D), (what, labels.count, len(D))
    fx = None if fixed is None else volume_of(fixed, depth)
    dst = volume_of(base, depth)
    if device_memory:
        import torch
        t_off = torch.full((max(len(D), 1), 3), 77, dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        st = labels.fallDevice(t_off.data_ptr(), fx, direction, limit)
        with Stream() as stream:
            labels.placeDevice(t_off.data_ptr(), dst, vrc.capi.VRC_COPY_OR, None, stream)
            placed = dst.download()                     # ordered behind the device-memory place: it is dst's last edit
        offsets = t_off.cpu().numpy()[:len(D)]
    else:
        offsets, st = labels.fall(fx, direction, limit)
        assert labels.place(offsets, dst) is dst
        placed = dst.download()
    print(f"{what}: {len(D)} pieces, {int((D > 0).sum())} moved, max drop {int(D.max(initial=0))}, {st.rounds} rounds")
    assert offsets.dtype == np.int32 and np.array_equal(offsets, want), what
    assert model.stats_tuple(st) == model.stats(ids, D), what
    assert (1 <= st.rounds <= len(D) + 1 if len(D) else st.rounds == 0) and tuple(st.reserved) == (0, 0), (what, st.rounds)
    assert np.array_equal(placed, model.place(ids, want, base)), what
    for v in (fx, dst):
        if v is not None:
            v.close()
    labels.close()
    return D, st


# ---- random debris over random fixed voxels ---------------------------------------------------------------------

@pytest.mark.parametrize("S,connectivity,direction,limit,seed", model.RANDOM_CASES)
def test_random_cases(built, S, connectivity, direction, limit, seed):
    """all six directions, both connectivities, 16^3 and 32^3; the offsets in host memory for the even seeds and in device
    memory for the odd ones.  What the set covers: tests/test_volume_fall_host.py."""
    debris, fixed = model.random_case(S, seed)
    check_fall(debris, fixed, connectivity, direction, limit, device_memory=bool((seed + direction) & 1), what=(S, connectivity, direction, limit))


# ---- constructed cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", range(6))
def test_plate_stack_and_hooked_shapes(built, direction):
    """six plates with gaps 1 .. 5 in a staircase, a chain of piece-on-piece constraints, and two C shapes hooked into each
    other, a cycle of constraints"""
    debris, fixed = model.plate_stack(32, direction)
    D, st = check_fall(debris, fixed, 6, direction, what=("plates", direction))
    assert sorted(D.tolist()) == [1, 2, 4, 7, 11, 16]
    D, st = check_fall(debris, fixed, 26, direction, limit=5, what=("plates, limit 5", direction))
    assert sorted(D.tolist()) == [1, 2, 4, 5, 5, 5]
    D, st = check_fall(model.interlocked(16, direction), None, 26, direction, device_memory=True, what=("hooked", direction))
    assert sorted(D.tolist()) == [3, 4]


@pytest.mark.parametrize("direction", range(6))
def test_wall_fixed_null_and_through_empty(built, direction):
    """a piece already on the wall, a piece whose bottom voxel sits in F (and one that does not, above it), fixed = NULL,
    and labels made through the EMPTY voxels: the pieces are then the pockets of air in a solid block"""
    S = 16
    axis, side = direction >> 1, direction & 1
    g = model.step_of(direction)

    def cell(q, a, b):
        p = [0, 0, 0]
        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = (S - 1 - q if side else q), a, b
        return tuple(p)
    debris = np.zeros((S, S, S), np.uint8)
    fixed = np.zeros((S, S, S), np.uint8)
    for q in (0, 1, 2):
        debris[cell(q, 3, 3)] = 1                       # on the wall
    for q in (5, 6):
        debris[cell(q, 3, 3)] = 1                       # above it, two cells of air between
    for q in (4, 5, 6):
        debris[cell(q, 9, 7)] = 1                       # its bottom voxel in F
    fixed[cell(4, 9, 7)] = 1
    for q in (9, 10):
        debris[cell(q, 9, 7)] = 1                       # above that one: falls 2
    debris[cell(12, 12, 12)] = 1                        # over a cell of F further on
    fixed[cell(7, 12, 12)] = 1
    ids = components_model.label(debris, 6)[0]
    D, st = check_fall(debris, fixed, 6, direction, ids=ids, what=("constructed", direction))
    by_voxel = {name: int(D[ids[c]]) for name, c in (("wall", cell(0, 3, 3)), ("above", cell(5, 3, 3)), ("in_f", cell(4, 9, 7)),
                                                      ("over", cell(9, 9, 7)), ("speck", cell(12, 12, 12)))}
    assert by_voxel == {"wall": 0, "above": 2, "in_f": 0, "over": 2, "speck": 4}, by_voxel
    D, st = check_fall(debris, None, 6, direction, ids=ids, what=("fixed = NULL", direction))
    assert int(D[ids[cell(4, 9, 7)]]) == 4 and int(D[ids[cell(12, 12, 12)]]) == 12
    # through the empty voxels: the volume is solid but for three pockets, which "fall" through the solid
    block = 1 - debris
    D, st = check_fall(block, fixed, 6, direction, through_empty=True, what=("through empty", direction))
    assert len(D) == 5 and int(D.max()) == 4
    assert g[axis] == (1 if side else -1)


def test_no_pieces(built):
    import cpuvoxelraycaster_amd as vrc
    L = vrc.capi.load()
    empty = vrc.VoxelVolume(4)
    labels = empty.labelComponents(6)
    floor = vrc.VoxelVolume(4)
    floor.fillBoxes([[0, 0, 0, 16, 2, 16]])
    offsets, st = labels.fall(floor, vrc.capi.VRC_FACE_YN)
    assert offsets.shape == (0, 3) and bytes(st) == bytes(32)
    canary = np.full(3, 5, np.int32)
    assert L.vrc_fall_drops(labels._h, None, 3, 0, vrc.capi.ptr(canary), vrc.capi.VRC_MEM_HOST, None) == 0 and (canary == 5).all()
    assert labels.place(offsets, floor) is floor and floor.solidCount() == 512
    assert L.vrc_fall_place(labels._h, None, None, floor._h, vrc.capi.VRC_COPY_ANDNOT, vrc.capi.VRC_MEM_DEVICE, None) == 0
    assert floor.solidCount() == 512
    for v in (labels, floor, empty):
        v.close()


@pytest.mark.parametrize("direction", range(6))
def test_word_and_brick_borders_at_64(built, direction):
    """64^3: boxes of odd size across brick borders (odd coordinates), word borders (z = 7 | 8, 31 | 32) and the 32-voxel border
    on every axis, some over ledges of F; every column is one whole 64-lane chunk"""
    S = 64
    debris = np.zeros((S, S, S), np.uint8)
    fixed = np.zeros((S, S, S), np.uint8)
    for lo, size in [((29, 29, 29), (5, 5, 5)), ((5, 6, 5), (3, 3, 5)), ((40, 7, 30), (3, 9, 3)), ((7, 41, 6), (9, 2, 3)), ((50, 50, 13), (1, 1, 7)),
                     ((30, 12, 50), (4, 3, 3)), ((12, 30, 55), (3, 5, 2)), ((55, 31, 31), (2, 2, 2)), ((31, 55, 7), (2, 3, 2)), ((20, 20, 40), (7, 7, 1))]:
        debris[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = 1
    for lo, size in [((0, 0, 0), (64, 2, 1)), ((31, 31, 60), (3, 3, 2)), ((60, 28, 28), (2, 4, 4)), ((28, 1, 28), (4, 2, 4)), ((2, 30, 30), (1, 3, 3))]:
        fixed[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = 1
    fixed[debris != 0] = 0
    D, st = check_fall(debris, fixed, 26, direction, device_memory=bool(direction & 1), what=("64^3", direction))
    assert len(D) == 10 and (D > 0).all()


@pytest.mark.parametrize("direction", range(6))
def test_columns_longer_than_a_chunk_at_128(built, direction):
    """128^3, where a column is two 64-cell chunks: boxes in the far chunk whose nearest obstacle -- the wall, a ledge of F,
    another piece -- lies in the near one, and a bar that spans both.  The ids are analytic: the boxes do not touch, and a
    piece's id is the rank of its first voxel's key."""
    import cpuvoxelraycaster_amd as vrc
    S, depth = 128, 7
    axis, side = direction >> 1, direction & 1

    def box(q0, q1, a0, a1, b0, b1):
        lo_hi = [0] * 6
        for ax, (u, v) in ((axis, (S - q1, S - q0) if side else (q0, q1)), ((axis + 1) % 3, (a0, a1)), ((axis + 2) % 3, (b0, b1))):
            lo_hi[ax], lo_hi[3 + ax] = u, v
        return lo_hi
    pieces = [box(70, 75, 10, 15, 10, 15),          # nothing ahead: the wall, 70 cells on
              box(100, 103, 12, 20, 12, 14),        # rests on the first: 25 cells of air between
              box(90, 92, 40, 43, 40, 47),          # a ledge of F at 30 .. 31 ahead: falls 58
              box(65, 66, 63, 65, 63, 65),          # a piece at 62 .. 63 ahead, the chunk border between them
              box(62, 64, 63, 65, 64, 65),
              box(20, 120, 100, 101, 101, 102)]     # a bar across both chunks
    ledges = [box(30, 32, 41, 42, 41, 42), box(3, 5, 63, 64, 64, 65)]
    want = [70, 70 + 25, 58, 57 + 1, 57, 20]            # the fifth: 57 cells of air down to the ledge at 3 .. 4
    medium, fx = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
    medium.fillBoxes(pieces)
    fx.fillBoxes(ledges)
    labels = medium.labelComponents(6)
    rec = labels.components()
    assert labels.count == 6
    order = {tuple(int(v) for v in r["lo"]): i for i, r in enumerate(rec)}
    D = np.array([0] * 6, np.int64)
    for b, d in zip(pieces, want):
        D[order[tuple(b[:3])]] = d
    offsets, st = labels.fall(fx, direction)
    assert np.array_equal(offsets, model.offsets_of(D, direction)), (offsets.tolist(), D.tolist())
    assert 1 <= st.rounds <= 7 and st.pieces == 6 and st.moved_pieces == 6 and st.max_drop == 95
    assert st.moved_voxels == int(rec["voxels"].sum()) == medium.solidCount()
    labels.place(offsets, fx)
    moved = [[b[a] + int(offsets[order[tuple(b[:3])], a % 3]) for a in range(6)] for b in pieces]
    assert fx.solidCount() == int(rec["voxels"].sum()) + 2 * 1 + 2 * 1
    assert [int(v) for v in fx.countBoxes(moved)] == [int(rec[order[tuple(b[:3])]]["voxels"]) for b in pieces]
    for v in (labels, medium, fx):
        v.close()


# ---- place ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scattered():
    """a 32^3 volume of a few dozen pieces with its model labelling, shared and left unchanged"""
    debris, _ = model.random_case(32, 4242)
    ids, rec = components_model.label(debris, 6)
    assert len(rec) > 20
    return debris, ids, rec


def test_place_any_offsets(built, scattered):
    """offsets of any sign, some pushing part of a piece or all of it out of the volume, some beyond 2^20 (dropped whole),
    many pieces onto the same voxels; OR and ANDNOT; a keep mask and NULL keep; dst the medium itself; REPLACE refused"""
    import cpuvoxelraycaster_amd as vrc
    capi = vrc.capi
    debris, ids, rec = scattered
    S, n = 32, len(rec)
    rng = np.random.default_rng(5)
    content = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    medium = volume_of(debris, 5)
    labels = medium.labelComponents(6)
    assert labels.count == n
    off = rng.integers(-12, 13, (n, 3)).astype(np.int32)
    off[0] = (0, 0, (1 << 20) + 1)
    off[1] = (-(1 << 20) - 1, 0, 0)
    off[2] = (1 << 20, 0, 0)                            # within the limit: simply outside the volume
    off[3] = (-2 ** 31, 2 ** 31 - 1, 0)
    to_one_spot = (np.array([16, 16, 16]) - rec["lo"].astype(np.int64)).astype(np.int32)
    keep = (rng.random(n) < 0.5).astype(np.uint8) * 3
    for offsets in (off, to_one_spot, np.zeros((n, 3), np.int32)):
        for k in (None, keep):
            for op_or in (True, False):
                op = capi.VRC_COPY_OR if op_or else capi.VRC_COPY_ANDNOT
                dst = volume_of(content, 5)
                labels.place(offsets, dst, op, k)
                assert np.array_equal(dst.download(), model.place(ids, offsets, content, op_or, k)), (op_or, k is None)
                dst.close()
    fresh = labels.place(to_one_spot)                   # a new volume
    assert np.array_equal(fresh.download(), model.place(ids, to_one_spot, np.zeros_like(content)))
    assert fresh.solidCount() < int(debris.sum())       # pieces landed on each other
    fresh.close()
    for op_or in (True, False):                         # dst is the medium the labels were made from: the labels are a snapshot
        itself = volume_of(debris, 5)
        own = itself.labelComponents(6)
        own.place(off, itself, capi.VRC_COPY_OR if op_or else capi.VRC_COPY_ANDNOT)
        assert np.array_equal(itself.download(), model.place(ids, off, debris, op_or))
        own.close()
        itself.close()
    with pytest.raises(vrc.VrcError, match="vrc_fall_place: VRC_COPY_REPLACE"):
        labels.place(off, medium, capi.VRC_COPY_REPLACE)
    assert np.array_equal(medium.download(), debris)
    labels.close()
    medium.close()


def test_two_calls_give_identical_bytes(built, scattered):
    import cpuvoxelraycaster_amd as vrc
    debris, ids, rec = scattered
    _, fixed = model.random_case(32, 4243)
    medium, fx = volume_of(debris, 5), volume_of(fixed, 5)
    labels = medium.labelComponents(6)
    scratch = fx.editScratchBytes()
    results = []
    for _ in range(2):
        offsets, st = labels.fall(fx, vrc.capi.VRC_FACE_ZN)
        dst = labels.place(offsets)
        results.append((offsets.tobytes(), model.stats_tuple(st), dst.download().tobytes()))
        dst.close()
    assert results[0] == results[1]
    assert fx.editScratchBytes() == scratch            # the fall keeps nothing on the volume
    for v in (labels, medium, fx):
        v.close()


# ---- dropLoose --------------------------------------------------------------------------------------------------

def scene_32():
    """a slab, a pillar on it whose middle a sphere has dug out, and a floating block; down is -y"""
    S = 32
    vol = np.zeros((S, S, S), np.uint8)
    vol[:, 0:3, :] = 1
    vol[14:18, 3:28, 14:18] = 1
    x, y, z = np.indices((S, S, S))
    vol[(x - 16) ** 2 + (y - 12) ** 2 + (z - 16) ** 2 <= 25] = 0
    vol[4:9, 20:23, 5:12] = 1
    return vol


def test_drop_loose(built):
    import cpuvoxelraycaster_amd as vrc
    S = 32
    vol = scene_32()
    anchor = [[0, 0, 0, S, 1, S]]
    whole, _ = components_model.label(vol, 6)
    supported = (whole == whole[0, 0, 0]).astype(np.uint8)
    debris = vol & (1 - supported)
    ids, rec = components_model.label(debris, 6)
    assert len(rec) == 2 and int(supported.sum()) > 3 * S * S
    D = model.drops(ids, supported, vrc.capi.VRC_FACE_YN)
    want = model.place(ids, model.offsets_of(D, vrc.capi.VRC_FACE_YN), supported)
    assert (D > 0).all() and int(want.sum()) == int(vol.sum())

    world = vrc.VoxelVolume(5)
    world.fillBoxes([[0, 0, 0, S, 3, S], [14, 3, 14, 18, 28, 18]])
    world.fillSpheres([[16, 12, 16, 5]], False)
    world.fillBoxes([[4, 20, 5, 9, 23, 12]])
    assert np.array_equal(world.download(), vol)
    before = world.solidCount()
    st = world.dropLoose(anchor, vrc.capi.VRC_FACE_YN)
    assert model.stats_tuple(st) == model.stats(ids, D) and 1 <= st.rounds <= 3
    assert world.solidCount() == before
    assert np.array_equal(world.download(), want)
    svo = world.commit()
    assert svo.n_nodes > 0
    svo.close()
    # settled: every piece of the result rests, through a chain of pieces, on the slab at the wall
    labels = world.labelComponents(6)
    offsets, again = labels.fall(None, vrc.capi.VRC_FACE_YN)
    assert labels.count == 1 and not offsets.any() and again.moved_pieces == 0 and again.max_drop == 0
    labels.close()
    # with a limit of 2 the pieces hang in the air, and a second call lets them go on
    world.close()
    world = volume_of(vol, 5)
    st = world.dropLoose(anchor, vrc.capi.VRC_FACE_YN, 6, 2)
    D2 = model.drops(ids, supported, vrc.capi.VRC_FACE_YN, 2)
    assert st.max_drop == 2 and np.array_equal(world.download(), model.place(ids, model.offsets_of(D2, vrc.capi.VRC_FACE_YN), supported))
    world.close()
