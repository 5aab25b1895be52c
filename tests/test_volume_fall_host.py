"""Falling pieces on a machine without a GPU: the yardstick of the GPU tests itself -- the tick simulation of
tests/fall_model.py against the column relaxation taken literally from the rule of include/vrc.h, a different algorithm --,
the case generators of the GPU tests under the model alone, the refusals that need no device, the stats record's size and
the C++ host adapter under a plain C++14 compiler."""
import ctypes as C
import os

import numpy as np
import pytest

import components_model
import fall_model as model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = model.NONE


def relax_literally(ids, fixed, direction, drop_limit=0):
    """The rule as written, voxel by voxel and k by k: D starts above every bound and is lowered until every constraint of
    every voxel holds -- the greatest solution."""
    S = ids.shape[0]
    g = [int(v) for v in model.step_of(direction)]
    voxels = [(int(ids[x, y, z]), (x, y, z)) for x, y, z in np.argwhere(ids != NONE).tolist()]
    C_ = max((i for i, _ in voxels), default=-1) + 1
    D = [drop_limit if drop_limit else 10 ** 9] * C_
    F = np.zeros((S, S, S), bool) if fixed is None else np.asarray(fixed) != 0
    changed = True
    while changed:
        changed = False
        for i, v in voxels:
            bound = D[i]
            if F[v]:
                bound = 0
            k = 1
            while True:
                w = (v[0] + k * g[0], v[1] + k * g[1], v[2] + k * g[2])
                if min(w) < 0 or max(w) >= S:
                    bound = min(bound, k - 1)           # rule 1: v + D g inside the volume
                    break
                if F[w]:
                    bound = min(bound, k - 1)
                j = int(ids[w])
                if j != NONE and j != i:
                    bound = min(bound, D[j] + k - 1)
                k += 1
            if bound < D[i]:
                D[i] = bound
                changed = True
    return np.array(D, np.int64)


def rounds_in_column_order(ids, fixed, direction):
    """Rounds of the device's pass run sequentially, the columns in ascending order and each from the far face backwards
    with only the nearest non-empty voxel ahead, in place: (D, rounds issued, the last one changing nothing)"""
    S = ids.shape[0]
    axis, side = direction >> 1, direction & 1
    F = np.zeros((S, S, S), bool) if fixed is None else np.asarray(fixed) != 0
    big = 1 << 40
    D = np.full(int(ids[ids != NONE].max()) + 1, big, np.int64)
    rounds = 0
    while True:
        rounds += 1
        changed = False
        for a in range(S):
            for b in range(S):
                pq, pj = -1, NONE
                for q in range(S):
                    p = [0, 0, 0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = (S - 1 - q if side else q), a, b
                    i, f = int(ids[tuple(p)]), bool(F[tuple(p)])
                    if i != NONE:
                        bound = 0 if f else None if pj == i else (q - pq - 1) + (0 if pj == NONE else int(D[pj]))
                        if bound is not None and bound < D[i]:
                            D[i], changed = bound, True
                    if f:
                        pq, pj = q, NONE
                    elif i != NONE:
                        pq, pj = q, i
        if not changed:
            return D, rounds


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("S", [4, 5, 6, 8])
def test_tick_simulation_against_the_rule(S, connectivity):
    """random pieces in 4^3 .. 8^3 (the model takes any S, the labelling model even ones: 5 is cut from 6), all six
    directions, drop_limit 0 / 1 / 3, F overlapping the pieces in a third of the cases"""
    rng = np.random.default_rng(50 + S + connectivity)
    moved = pieces = 0
    for trial in range(12):
        T = S + (S & 1)
        solid = np.zeros((T, T, T), np.uint8)
        solid[:S, :S, :S] = rng.random((S, S, S)) < (0.12 if connectivity == 26 else 0.25)
        ids = components_model.label(solid, connectivity)[0][:S, :S, :S]
        fixed = (rng.random((S, S, S)) < 0.1).astype(np.uint8)
        if trial % 3:
            fixed[ids != NONE] = 0
        for direction in range(6):
            for limit in (0, 1, 3):
                D = model.drops(ids, fixed if trial % 4 else None, direction, limit)
                want = relax_literally(ids, fixed if trial % 4 else None, direction, limit)
                assert np.array_equal(D, want), (S, connectivity, trial, direction, limit)
                # no two voxels share a cell after the move, and none has moved into F
                placed = np.argwhere(ids != NONE) + D[ids[ids != NONE].astype(np.int64), None] * model.step_of(direction)
                assert len(np.unique(placed, axis=0)) == len(placed) and placed.min(initial=0) >= 0 and placed.max(initial=0) < S
                out = model.place(ids, model.offsets_of(D, direction), np.zeros((S, S, S), np.uint8))
                assert int(out.sum()) == int((ids != NONE).sum())
                if trial % 4:
                    # a piece in F on entry stays; of the others no voxel ends in a cell of F
                    in_f = np.zeros(len(D), bool)
                    in_f[ids[(ids != NONE) & (fixed != 0)].astype(np.int64)] = True
                    assert (D[in_f] == 0).all()
                    clear = np.where(np.isin(ids, np.flatnonzero(in_f)), NONE, ids).astype(np.uint32)
                    assert not (model.place(clear, model.offsets_of(D, direction), np.zeros((S, S, S), np.uint8)) & fixed).any()
                moved += int((D > 0).sum())
                pieces += len(D)
    assert moved > 20 and pieces > moved


def test_model_place_and_stats():
    ids = np.full((8, 8, 8), NONE, np.uint32)
    ids[1:3, 1:3, 1:3] = 0
    ids[6, 6, 6] = 1
    ids[0, 7, 0] = 2
    off = np.array([[0, -1, 0], [3, 0, 0], [0, 0, model.OFFSET_LIMIT + 1]], np.int32)
    out = model.place(ids, off, np.zeros((8, 8, 8), np.uint8))
    assert int(out.sum()) == 8 and out[1:3, 0:2, 1:3].all()          # piece 1 leaves the volume, piece 2 is beyond the limit
    out = model.place(ids, off, np.ones((8, 8, 8), np.uint8), op_or=False, keep=[0, 1, 1])
    assert int(out.sum()) == 512
    out = model.place(ids, np.zeros((3, 3), np.int32), np.ones((8, 8, 8), np.uint8), op_or=False)
    assert int(out.sum()) == 512 - 10
    assert model.stats(ids, np.array([2, 0, 5])) == (9, 3, 2, 5)
    assert model.stats(np.full((4, 4, 4), NONE, np.uint32), np.zeros(0, np.int64)) == (0, 0, 0, 0)


def test_generators_meet_their_conditions():
    """the random set of the GPU test contains a piece that lands on another, a lower piece that falls farther than the
    one above it, a piece stopped by drop_limit and a piece held by F; the plate stack needs at least 3 rounds in column
    order; the hooked shapes fall 3 and 4"""
    found = set()
    for S, connectivity, direction, limit, seed in model.RANDOM_CASES:
        debris, fixed = model.random_case(S, seed)
        ids, rec = components_model.label(debris, connectivity)
        assert len(rec) >= 8
        D = model.drops(ids, fixed, direction, limit)
        found |= model.features(ids, fixed, direction, limit, D)
    assert found == {"lands_on_piece", "lower_falls_farther", "limit", "in_fixed"}, found
    for direction in range(6):
        debris, fixed = model.plate_stack(32, direction)
        ids, rec = components_model.label(debris, 26)
        assert len(rec) == 6
        D = model.drops(ids, fixed, direction)
        assert sorted(D.tolist()) == [1, 2, 4, 7, 11, 16]               # 1, then the gap to the plate ahead on top of its drop
        if direction in (0, 3, 4):
            got, rounds = rounds_in_column_order(ids, fixed, direction)
            assert np.array_equal(got, D) and 3 <= rounds <= len(D) + 1, rounds
        shape = model.interlocked(16, direction)
        ids, rec = components_model.label(shape, 26)
        assert len(rec) == 2
        assert sorted(model.drops(ids, None, direction).tolist()) == [3, 4]


def test_fall_stats_layout(built):
    from cpuvoxelraycaster_amd import capi
    assert C.sizeof(capi.FallStats) == 32
    assert [getattr(capi.FallStats, f).offset for f in ("moved_voxels", "pieces", "moved_pieces", "max_drop", "rounds", "reserved")] == [0, 8, 12, 16, 20, 24]


def test_fall_refusals_need_no_gpu(built):
    """NULL handles, a direction outside 0..5, a bad mem kind, an unknown op, REPLACE, a depth or device mismatch and NULL
    offsets with C > 0 are VRC_ERR_INVALID with the function's name before any HIP call: the handles here are not volumes or
    labels at all, and nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b, c = (C.c_uint32 * 128)(), (C.c_uint32 * 128)(), (C.c_uint32 * 128)()   # zero bytes: "depth 0, device 0, no pieces"
    pa, pb, pc = (C.cast(v, C.c_void_p) for v in (a, b, c))
    for i in range(128):
        c[i] = 0x01010101                                                     # every field differs, and as labels C > 0
    off = np.full(6, 7, np.int32)
    keep = np.ones(2, np.uint8)
    st = capi.FallStats()
    st.rounds = 99
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert L.vrc_fall_drops(None, pb, capi.VRC_FACE_YN, 0, capi.ptr(off), mem, C.byref(st)) == -1
        assert L.vrc_last_error().startswith(b"vrc_fall_drops: null labels")
        for direction in (-1, 6, 26):
            assert L.vrc_fall_drops(pa, pb, direction, 0, capi.ptr(off), mem, C.byref(st)) == -1
            assert L.vrc_last_error().startswith(b"vrc_fall_drops: direction"), L.vrc_last_error()
        assert L.vrc_fall_drops(pa, pc, capi.VRC_FACE_YN, 0, capi.ptr(off), mem, C.byref(st)) == -1
        assert L.vrc_last_error().startswith(b"vrc_fall_drops: labels"), L.vrc_last_error()
        assert L.vrc_fall_drops(pc, None, capi.VRC_FACE_YN, 0, None, mem, C.byref(st)) == -1
        assert L.vrc_last_error().startswith(b"vrc_fall_drops: null offsets"), L.vrc_last_error()
        assert st.rounds == 99
        assert L.vrc_fall_place(None, capi.ptr(keep), capi.ptr(off), pb, capi.VRC_COPY_OR, mem, None) == -1
        assert L.vrc_fall_place(pa, capi.ptr(keep), capi.ptr(off), None, capi.VRC_COPY_OR, mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_fall_place: null")
        for op in (-1, 3, 26):
            assert L.vrc_fall_place(pa, capi.ptr(keep), capi.ptr(off), pb, op, mem, None) == -1
            assert L.vrc_last_error().startswith(b"vrc_fall_place: bad op"), L.vrc_last_error()
        assert L.vrc_fall_place(pa, capi.ptr(keep), capi.ptr(off), pb, capi.VRC_COPY_REPLACE, mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_fall_place: VRC_COPY_REPLACE"), L.vrc_last_error()
        for op in (capi.VRC_COPY_OR, capi.VRC_COPY_ANDNOT):
            assert L.vrc_fall_place(pa, None, capi.ptr(off), pc, op, mem, None) == -1
            assert L.vrc_last_error().startswith(b"vrc_fall_place: labels"), L.vrc_last_error()
            assert L.vrc_fall_place(pc, None, None, pc, op, mem, None) == -1
            assert L.vrc_last_error().startswith(b"vrc_fall_place: null offsets"), L.vrc_last_error()
    for mem in (-1, 2, 7):
        assert L.vrc_fall_drops(pa, pb, capi.VRC_FACE_YN, 0, capi.ptr(off), mem, None) == -1
        assert L.vrc_fall_place(pa, None, capi.ptr(off), pb, capi.VRC_COPY_OR, mem, None) == -1
        assert b"bad mem kind" in L.vrc_last_error()
    # no pieces: legal without a device, zero stats, the offsets untouched -- with and without `fixed` and stats
    assert L.vrc_fall_drops(pa, pb, capi.VRC_FACE_ZP, 5, None, capi.VRC_MEM_HOST, C.byref(st)) == 0
    assert bytes(st) == bytes(32)
    assert L.vrc_fall_drops(pa, None, capi.VRC_FACE_XN, 0, capi.ptr(off), capi.VRC_MEM_DEVICE, None) == 0
    assert L.vrc_fall_place(pa, None, None, pb, capi.VRC_COPY_ANDNOT, capi.VRC_MEM_HOST, None) == 0
    assert not any(a) and not any(b) and all(v == 0x01010101 for v in c) and (off == 7).all()


def test_python_arguments(built):
    import cpuvoxelraycaster_amd as vrc
    labels = vrc.VoxelLabels(None, 2, 4, 0)
    with pytest.raises(TypeError, match="direction"):
        labels.fall()
    with pytest.raises(ValueError, match="offsets"):
        labels.place(np.zeros((3, 3), np.int32))
    with pytest.raises(ValueError, match="keep"):
        labels.place(np.zeros((2, 3), np.int32), keep=[1])


def test_host_adapter_with_fall_compiles(built):
    """HipVoxelLabels::fall / place and HipVoxelVolume::dropLoose in the header-only adapter: C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& debris) {\n'
           '    vrc_host::HipVoxelLabels labels = debris.labelComponents(6, false);\n'
           '    vrc_fall_stats st;\n'
           '    std::vector<int32_t> offsets = labels.fall(&world, VRC_FACE_YN, 0, &st);\n'
           '    labels.place(offsets, world, VRC_COPY_OR);\n'
           '    std::vector<uint8_t> keep(labels.count(), 1);\n'
           '    labels.place(offsets, world, VRC_COPY_ANDNOT, &keep);\n'
           '    const uint32_t anchor[6] = {0, 0, 0, 4, 1, 4};\n'
           '    vrc_fall_stats dropped = world.dropLoose(anchor, 1, VRC_FACE_YN, 26, 3);\n'
           '    return st.moved_voxels + dropped.moved_pieces + labels.fall(nullptr, VRC_FACE_ZP).size();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
