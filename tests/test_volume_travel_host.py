"""The travel-distance field on a machine without a GPU: the yardstick of the GPU tests itself -- the breadth-first model of
tests/travel_model.py against the definition taken literally (Bellman-Ford relaxation to a fixed point over explicit
neighbour lists, a different algorithm) --, the refusals that need no device, the stats record's size, and the C++ host
adapter with travelField / tracePaths under a plain C++14 compiler."""
import ctypes as C
import os

import numpy as np
import pytest

import travel_model as model
from volume_support import check_cpp_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = model.NONE


def bellman_ford(vol, seeds, connectivity, through_empty):
    """T(p) = min(T(p), T(q) + 1) over every ordered pair of neighbours (p, q) in M until nothing changes, as int64 with
    2^40 for "no chain"""
    S = vol.shape[0]
    M = (vol == 0) if through_empty else (vol != 0)
    big = np.int64(1) << 40
    T = np.where((seeds != 0) & M, 0, big).astype(np.int64).reshape(-1)
    index = lambda x, y, z: (x * S + y) * S + z
    pairs = []
    for x, y, z in np.argwhere(M):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    touching = (dx != 0) + (dy != 0) + (dz != 0)
                    if touching == 0 or (connectivity == 6 and touching != 1):
                        continue
                    qx, qy, qz = x + dx, y + dy, z + dz
                    if 0 <= qx < S and 0 <= qy < S and 0 <= qz < S and M[qx, qy, qz]:
                        pairs.append((index(x, y, z), index(qx, qy, qz)))
    if pairs:
        p, q = np.array(pairs, np.int64).T
        while True:
            before = T.copy()
            np.minimum.at(T, p, before[q] + 1)
            if np.array_equal(T, before):
                break
    return T.reshape(S, S, S)


def limited(T, step_limit):
    """the definition's third case: NONE where no chain exists or the least number exceeds the limit"""
    gone = (T >= np.int64(1) << 40) | ((T > step_limit) if step_limit else False)
    return np.where(gone, NONE, T).astype(np.uint32)


@pytest.mark.parametrize("through_empty", [False, True])
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("S", [4, 8])
def test_model_against_the_definition(S, connectivity, through_empty):
    rng = np.random.default_rng(4100 + S + connectivity + int(through_empty))
    for density in (0.05, 0.3, 0.5, 0.7, 0.0, 1.0):
        vol = (rng.random((S, S, S)) < density).astype(np.uint8)
        seeds = np.zeros((S, S, S), np.uint8)
        for x, y, z in rng.integers(0, S, (int(rng.integers(1, 6)), 3)):
            seeds[x, y, z] = 1
        literal = bellman_ford(vol, seeds, connectivity, through_empty)
        for step_limit in (0, 1, 3):
            T = model.field(vol, seeds, connectivity, through_empty, step_limit)
            want = limited(literal, step_limit)
            assert T.dtype == np.uint32 and np.array_equal(T, want), (S, connectivity, through_empty, density, step_limit)
            in_m = model.seeds_in_m(vol, seeds, through_empty)
            assert (T[in_m] == 0).all() and (T[~model.medium_set(vol, through_empty)] == NONE).all()
            n, reached, m, arg = model.stats(T, int(in_m.sum()))
            finite = want[want != NONE]
            assert (n, reached) == (int(in_m.sum()), len(finite))
            assert m == (int(finite.max()) if len(finite) else 0)
            if len(finite):
                assert want[arg] == m and not (want.reshape(-1)[:(arg[0] * S + arg[1]) * S + arg[2]] == m).any()
            else:
                assert arg == (0, 0, 0)


@pytest.mark.parametrize("S", [8, 16])
def test_model_through_open_air_is_manhattan_and_chebyshev(S):
    vol = np.zeros((S, S, S), np.uint8)
    seeds = np.zeros((S, S, S), np.uint8)
    where = (2, S - 1, S // 2)
    seeds[where] = 1
    d = np.abs(np.indices((S, S, S)) - np.array(where).reshape(3, 1, 1, 1))
    assert np.array_equal(model.field(vol, seeds, 6, True), d.sum(axis=0).astype(np.uint32))
    assert np.array_equal(model.field(vol, seeds, 26, True), d.max(axis=0).astype(np.uint32))
    assert (model.field(vol, seeds, 6, False) == NONE).all()          # the seed is not in M: nothing is solid


def test_model_trace_tie_break_and_select():
    S = 8
    vol = np.zeros((S, S, S), np.uint8)
    seeds = np.zeros((S, S, S), np.uint8)
    seeds[0, 0, 0] = 1
    T = model.field(vol, seeds, 6, True)
    length, route = model.trace(T, (1, 1, 1), 6)
    assert length == 3 and route.tolist() == [[1, 1, 1], [0, 1, 1], [0, 0, 1], [0, 0, 0]]      # -x before -y before -z
    T26 = model.field(vol, seeds, 26, True)
    assert model.trace(T26, (2, 2, 1), 26)[1].tolist() == [[2, 2, 1], [1, 1, 0], [0, 0, 0]]
    assert model.trace(T, (3, 0, 0), 6, capacity=2)[1].tolist() == [[3, 0, 0], [2, 0, 0]]
    assert model.trace(T, (3, 0, 0), 6, capacity=0)[0] == 3 and len(model.trace(T, (3, 0, 0), 6, capacity=0)[1]) == 0
    assert model.trace(T, (S, 0, 0), 6)[0] == NONE and len(model.trace(T, (S, 0, 0), 6)[1]) == 0
    assert int(model.select(T, 0, 1).sum()) == 4 and int(model.select(T, NONE, NONE).sum()) == 0
    assert [o for o in model.offsets(6)] == [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)]


def test_travel_stats_layout(built):
    from cpuvoxelraycaster_amd import capi
    assert C.sizeof(capi.TravelStats) == 40
    assert [getattr(capi.TravelStats, f).offset for f in ("seeds", "reached", "max_steps", "argmax", "sweeps", "reserved")] == [0, 8, 16, 20, 32, 36]
    hdr = os.path.join(ROOT, "include", "vrc.h")
    src = '#include "%s"\nstatic_assert(sizeof(vrc_travel_stats) == 40, "vrc_travel_stats");\nint main() { return 0; }\n' % hdr
    check_cpp_syntax(src)


def test_travel_refusals_need_no_gpu(built):
    """NULL handles, a connectivity other than 6 / 26, a `through` other than 0 / 1, a depth mismatch, a depth outside 2..10
    and a NULL `out` are VRC_ERR_INVALID with the function's name before any HIP call: the handles here are not volumes or
    fields at all, and nothing is written."""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    a, b = (C.c_uint32 * 128)(), (C.c_uint32 * 128)()        # 512 zero bytes each: "depth 0 on device 0" whatever the layout
    pa, pb = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    out, stats = C.c_void_p(0x55), capi.TravelStats()
    stats.max_steps = 7
    field = L.vrc_travel_field
    cases = [(None, pa, 6, 0, C.byref(out), b": null"), (pa, None, 6, 0, C.byref(out), b": null"), (pa, pa, 6, 0, None, b": null"),
             (pa, pa, 0, 0, C.byref(out), b": connectivity"), (pa, pa, 18, 1, C.byref(out), b": connectivity"),
             (pa, pa, 6, 2, C.byref(out), b": bad through"), (pa, pa, 26, -1, C.byref(out), b": bad through"),
             (pa, pa, 6, 0, C.byref(out), b": depth 0 not in [2,10]"), (pa, pa, 26, 1, C.byref(out), b": depth 0 not in [2,10]")]
    for seeds, medium, connectivity, through, o, text in cases:
        for limit in (0, 5):
            for st in (None, C.byref(stats)):
                assert field(seeds, medium, connectivity, through, limit, o, st) == -1, text
                assert L.vrc_last_error().startswith(b"vrc_travel_field" + text), L.vrc_last_error()
    for i in range(128):
        b[i] = 0x01010101                                    # every field differs from a's: a depth (or device) mismatch
    for first, second in ((pa, pb), (pb, pa)):
        assert field(first, second, 6, 0, 0, C.byref(out), C.byref(stats)) == -1
        assert L.vrc_last_error().startswith(b"vrc_travel_field: volumes o"), L.vrc_last_error()
    assert out.value == 0x55 and stats.max_steps == 7 and stats.seeds == 0 and stats.sweeps == 0
    assert not any(a) and all(v == 0x01010101 for v in b)

    # routes: a NULL field, a Euclidean one (the zero bytes say connectivity 0), then -- on a record that claims to be a
    # travel field -- a bad mem kind and missing buffers
    xyz, lengths, paths = np.zeros(3, np.uint32), np.full(1, 9, np.uint32), np.full(6, 9, np.uint32)
    trace = L.vrc_travel_trace_paths
    assert L.vrc_travel_connectivity(None) == 0 and L.vrc_travel_connectivity(pa) == 0
    for mem in (capi.VRC_MEM_HOST, capi.VRC_MEM_DEVICE):
        assert trace(None, 1, capi.ptr(xyz), 2, capi.ptr(paths), capi.ptr(lengths), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_travel_trace_paths: null"), L.vrc_last_error()
        assert trace(pa, 1, capi.ptr(xyz), 2, capi.ptr(paths), capi.ptr(lengths), mem, None) == -1
        assert L.vrc_last_error().startswith(b"vrc_travel_trace_paths: not a travel field"), L.vrc_last_error()
    for i in range(128):
        b[i] = 6                                             # device 6, depth 6, connectivity 6: refused before any of it is used
    assert L.vrc_travel_connectivity(pb) == 6
    for mem in (-1, 2, 7):
        assert trace(pb, 1, capi.ptr(xyz), 2, capi.ptr(paths), capi.ptr(lengths), mem, None) == -1
        assert b"bad mem kind" in L.vrc_last_error()
    assert trace(pb, 1, None, 2, capi.ptr(paths), capi.ptr(lengths), capi.VRC_MEM_HOST, None) == -1
    assert trace(pb, 1, capi.ptr(xyz), 2, capi.ptr(paths), None, capi.VRC_MEM_HOST, None) == -1
    assert trace(pb, 1, capi.ptr(xyz), 2, None, capi.ptr(lengths), capi.VRC_MEM_HOST, None) == -1
    assert L.vrc_last_error().startswith(b"vrc_travel_trace_paths: null paths"), L.vrc_last_error()
    assert trace(pb, 0, None, 0, None, None, capi.VRC_MEM_HOST, None) == 0          # no starts: nothing to do
    assert lengths[0] == 9 and (paths == 9).all()


def test_python_refusals_before_any_device_call(built):
    import cpuvoxelraycaster_amd as vrc
    volume = vrc.VoxelVolume.__new__(vrc.VoxelVolume)
    volume._h, volume.depth, volume.device = None, 5, 0
    with pytest.raises(ValueError):
        volume.reachableWithin(volume, -1)


def test_host_adapter_with_travel_compiles(built):
    """HipVoxelVolume::travelField and HipVoxelDistance::tracePaths / connectivity / travelStats in the header-only adapter:
    C++14, no GLM, no HIP headers."""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& seeds) {\n'
           '    vrc_host::HipVoxelDistance field = world.travelField(seeds, VRC_CONNECT_ALL, true, 40);\n'
           '    const vrc_travel_stats& stats = field.travelStats();\n'
           '    vrc_host::HipVoxelVolume near(world.depth());\n'
           '    field.select(0, 10, near, VRC_COPY_REPLACE);\n'
           '    const uint32_t xyz[3] = {1, 2, 3};\n'
           '    std::vector<uint32_t> paths, lengths;\n'
           '    field.tracePaths(xyz, 1, 8, paths, lengths);\n'
           '    vrc_host::HipVoxelDistance self = world.travelField(world);\n'
           '    return stats.seeds + stats.reached + stats.max_steps + stats.sweeps + paths.size() + lengths[0] + field.connectivity() + self.depth();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)


def test_travel_refusal_texts(built):
    """the WHOLE vrc_last_error() text of every refusal decided before the first HIP call, as literals"""
    from cpuvoxelraycaster_amd import capi
    L = capi.load()

    def handle(fill=0, **words):
        block = (C.c_uint32 * 128)(*([fill] * 128))
        for name, value in words.items():
            block[int(name[1:])] = value
        return block

    zero, other, ones, device_1 = handle(), handle(), handle(0x01010101), handle(w0=1)
    travel_6 = handle(w2=6)          # vrc_distance::connectivity is the third 32-bit member: a travel field made with 6 neighbours
    p = lambda block: C.cast(block, C.c_void_p)
    out = C.c_void_p(0x55)
    u32, u64 = np.zeros(16, np.uint32), np.zeros(8, np.uint64)
    name = "vrc_travel_field"
    cases = [(name, (None, p(other), 6, 0, 0, C.byref(out), None), "null volume"),
             (name, (p(zero), None, 6, 0, 0, C.byref(out), None), "null volume"),
             (name, (p(zero), p(other), 6, 0, 0, None, None), "null argument"),
             (name, (p(zero), p(other), 18, 0, 0, C.byref(out), None), "connectivity 18 is neither 6 nor 26"),
             (name, (p(zero), p(other), 26, 2, 0, C.byref(out), None), "bad through 2"),
             (name, (p(zero), p(ones), 6, 1, 7, C.byref(out), None), "volumes of depths 0 and 16843009"),
             (name, (p(zero), p(device_1), 6, 1, 0, C.byref(out), None), "volumes on devices 0 and 1"),
             (name, (p(zero), p(zero), 26, 0, 0, C.byref(out), None), "depth 0 not in [2,10]"),
             # two refusals at once: the one that wins
             (name, (p(zero), p(ones), 18, 0, 0, C.byref(out), None), "connectivity 18 is neither 6 nor 26"),
             (name, (p(zero), p(device_1), 26, 2, 0, C.byref(out), None), "bad through 2"),
             (name, (p(ones), p(device_1), 6, 1, 0, C.byref(out), None), "volumes of depths 16843009 and 0"),
             (name, (p(device_1), p(zero), 6, 0, 0, C.byref(out), None), "volumes on devices 1 and 0"),
             (name, (p(zero), p(zero), 7, 0, 0, C.byref(out), None), "connectivity 7 is neither 6 nor 26")]
    name = "vrc_travel_trace_paths"
    too_many = 0x7FFFFFFF * 256 + 1
    cases += [(name, (None, 1, capi.ptr(u32), 4, capi.ptr(u32), capi.ptr(u64), 0, None), "null distance field"),
              (name, (p(zero), 1, capi.ptr(u32), 4, capi.ptr(u32), capi.ptr(u64), 0, None), "not a travel field (a Euclidean field has no routes)"),
              (name, (p(travel_6), 1, capi.ptr(u32), 4, capi.ptr(u32), capi.ptr(u64), 2, None), "bad mem kind 2"),
              (name, (p(travel_6), 1, None, 4, capi.ptr(u32), capi.ptr(u64), 0, None), "null buffer"),
              (name, (p(travel_6), 1, capi.ptr(u32), 4, capi.ptr(u32), None, 1, None), "null buffer"),
              (name, (p(travel_6), 1, capi.ptr(u32), 4, None, capi.ptr(u64), 0, None), "null paths with capacity 4"),
              (name, (p(travel_6), too_many, capi.ptr(u32), 4, capi.ptr(u32), capi.ptr(u64), 0, None), "too many starts for one launch")]
    for name, args, text in cases:
        assert getattr(L, name)(*args) == -1, (name, text)
        assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
        assert not any(zero) and not any(other) and all(v == 0x01010101 for v in ones) and list(device_1) == [1] + [0] * 127
        assert list(travel_6) == [0, 0, 6] + [0] * 125 and not u32.any() and not u64.any() and out.value == 0x55
