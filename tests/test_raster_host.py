"""Surface voxelisation without a GPU: the numpy model (raster_model.py) held to facts that do not come from the predicate -- a
box's shell, a diagonal's supercover, the faces of a voxel field, the theorem that ties the thin shell to the crossing parity of
vrc_volume_xor_mesh, sampled points of triangles -- the pruning of csrc/vrc_raster.h held to the predicate by brute force in a
sanitized stand-alone program, every refusal that precedes a device call by its whole text, the symbol, the constants and the
wrappers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raster_model as model
import stamp_model
import surface_model
import voxelize_model
from volume_support import ROOT, check_cpp_syntax

U = model.UNIT


def as_set(p):
    return set(map(tuple, np.asarray(p).reshape(-1, 3).tolist()))


def clipped_box(S, lo, hi):
    """the voxels of [lo, hi) inside the volume, as a bool field"""
    f = np.zeros((S, S, S), bool)
    l, h = [max(0, q) for q in lo], [min(S, q) for q in hi]
    if all(a < b for a, b in zip(l, h)):
        f[l[0]:h[0], l[1]:h[1], l[2]:h[2]] = True
    return f


def random_triangles(rng, S, count):
    """triangles around a volume of S^3: general ones, small ones, degenerate ones, ones on multiples of 32"""
    return np.concatenate([rng.integers(-U, U * S + U, (count // 2, 9)), model.small_triangles(rng, S, count - count // 2)])


# ---- 1. facts that do not come from the predicate --------------------------------------------------------------------

@pytest.mark.parametrize("lo,hi", [((3, 4, 5), (7, 6, 11)), ((0, 2, 1), (5, 16, 3)), ((-2, 5, 5), (4, 9, 20)), ((6, 6, 6), (7, 7, 7))])
def test_touched_of_a_box_is_its_shell(lo, hi):
    S = 16
    tris = model.box_mesh(U * np.array(lo), U * np.array(hi))
    want = clipped_box(S, [q - 1 for q in lo], [q + 1 for q in hi]) & ~clipped_box(S, [q + 1 for q in lo], [q - 1 for q in hi])
    assert np.array_equal(model.selected(S, tris, model.TOUCHED), want)


@pytest.mark.parametrize("k", [0, 1, 5, 16, 20])
def test_touched_of_a_diagonal_segment_is_its_supercover(k):
    S = 16
    t = [0, 0, 0] + [U * k] * 6
    want = np.zeros((S, S, S), bool)
    for i in range(k + 1):
        want |= clipped_box(S, [i - 1] * 3, [i + 1] * 3)
    for perm in ([0, 1, 2], [1, 2, 0], [1, 0, 2]):                             # whichever vertex is the lone one
        tri = np.array(t).reshape(3, 3)[perm].reshape(9)
        assert np.array_equal(model.selected(S, [tri], model.TOUCHED), want), perm


def test_a_triangle_in_a_centre_plane_stays_in_its_slab():
    S = 16
    rng = np.random.default_rng(5)
    for axis in range(3):
        for j in (0, 7, 15):
            for _ in range(10):
                t = rng.integers(-U, U * S + U, (3, 3))
                t[:, axis] = U * j + model.HALF
                p = model.touched_voxels(S, t.reshape(9))
                assert len(p) > 0 and (p[:, axis] == j).all()
                q = model.thin_voxels(S, t.reshape(9))
                assert (q[:, axis] == j).all()


def test_thin_of_a_field_s_faces():
    """the closed face mesh of a field V: along each axis the crossing between a voxel and its -a neighbour lies on the boundary
    and goes to the upper voxel, so THIN is exactly the voxels whose state differs from their -a neighbour's (outside = empty)"""
    S = 16
    rng = np.random.default_rng(11)
    for density in (0.1, 0.5, 0.9):
        V = rng.random((S, S, S)) < density
        tris = surface_model.triangles(surface_model.faces(V, closed=True))
        want = np.zeros((S, S, S), bool)
        for a in range(3):
            below = np.roll(V, 1, axis=a)
            first = [slice(None)] * 3
            first[a] = 0
            below[tuple(first)] = False
            want |= V != below
        assert np.array_equal(model.selected(S, tris, model.THIN), want), density


def turned(tris, perm, flip, size):
    """vertices q_a = p[perm[a]], mirrored in [0, size] where flip[a] is set"""
    t = np.asarray(tris, np.int64).reshape(-1, 3, 3)
    out = np.empty_like(t)
    for a in range(3):
        out[:, :, a] = size - t[:, :, perm[a]] if flip[a] else t[:, :, perm[a]]
    return out.reshape(-1, 9)


def closed_meshes():
    """seeded closed meshes in a volume of 16^3: the surface of a random 8^3 field, turned by a quarter turn or a mirror and
    offset by a vector that is no multiple of 64 (partly outside the volume for some)"""
    rng = np.random.default_rng(23)
    turns = stamp_model.all_signed_permutations()
    for i in range(12):
        V = rng.random((8, 8, 8)) < (0.3, 0.6)[i % 2]
        tris = surface_model.triangles(surface_model.faces(V, closed=True)).astype(np.int64)
        perm, flip = turns[int(rng.integers(0, len(turns)))]
        offset = rng.integers(-100, 9 * U, 3)
        offset += (offset % U == 0)
        yield turned(tris, perm, flip, 8 * U) + np.tile(offset, 3)


def test_thin_shell_separates_what_xor_mesh_separates():
    """the theorem of include/vrc.h: wherever two voxels adjacent along a differ in the crossing parity read along a, one of the
    two is in the thin shell"""
    S = 16
    pairs = 0
    for tris in closed_meshes():
        thin = model.selected(S, tris, model.THIN)
        for a in range(3):
            u, v = (a + 1) % 3, (a + 2) % 3
            moved = tris.reshape(-1, 3, 3)[:, :, [u, v, a]].reshape(-1, 9)      # a becomes z
            F = voxelize_model.xor_mesh(S, moved)                              # [p_u, p_v, p_a]
            state = np.transpose(F, np.argsort([u, v, a]))                      # [x, y, z]
            upper, lower = [slice(None)] * 3, [slice(None)] * 3
            upper[a], lower[a] = slice(1, S), slice(0, S - 1)
            differ = state[tuple(upper)] != state[tuple(lower)]
            either = thin[tuple(upper)] | thin[tuple(lower)]
            assert not (differ & ~either).any(), a
            pairs += int(differ.sum())
    assert pairs > 1000


def test_thin_is_part_of_touched_and_both_ignore_vertex_order():
    S = 12
    rng = np.random.default_rng(31)
    some_thin = 0
    for t in random_triangles(rng, S, 160):
        touched, thin = as_set(model.touched_voxels(S, t)), as_set(model.thin_voxels(S, t))
        assert thin <= touched, t
        some_thin += len(thin)
        for order in ([1, 2, 0], [2, 0, 1], [0, 2, 1], [1, 0, 2]):             # two rotations, two flips of the winding
            other = t.reshape(3, 3)[order].reshape(9)
            assert as_set(model.touched_voxels(S, other)) == touched, (t, order)
            assert as_set(model.thin_voxels(S, other)) == thin, (t, order)
    assert some_thin > 500


def test_a_triangle_beyond_the_limit_is_dropped():
    S = 8
    L = model.LIMIT
    kept = [-L, 0, 0, L, 0, 0, 0, L, U * S]
    assert len(model.touched_voxels(S, kept)) > 0 and len(model.thin_voxels(S, kept)) > 0
    for i in range(9):
        for excess in (L + 1, -L - 1):
            t = list(kept)
            t[i] = excess
            assert len(model.touched_voxels(S, t)) == 0 and len(model.thin_voxels(S, t)) == 0, t
    field = model.raster_mesh(S, [kept[:8] + [L + 1], [0, 0, 0, 64, 0, 0, 0, 64, 0]], model.TOUCHED)
    # the first is dropped.  The second lies in the plane z = 0 (layer -1 is outside) over voxel (0, 0) and reaches (1, 0) and
    # (0, 1) with its corners (64, 0) and (0, 64); voxel (1, 1) has x + y >= 128 and the triangle x + y <= 64
    assert as_set(np.argwhere(field)) == {(0, 0, 0), (1, 0, 0), (0, 1, 0)}


def test_touched_contains_the_voxels_of_sampled_points():
    """soundness by sampling: vertices on multiples of 8, so the points A + (i (B - A) + j (C - A)) / 8 are integers; every voxel
    whose closed cube holds such a point is selected"""
    S = 8
    rng = np.random.default_rng(47)
    checked = 0
    for _ in range(150):
        t = 8 * rng.integers(-8, 8 * S + 8, (3, 3))
        sel = model.selected(S, [t.reshape(9)], model.TOUCHED)
        for i in range(9):
            for j in range(9 - i):
                pt = t[0] + (i * (t[1] - t[0]) + j * (t[2] - t[0])) // 8
                assert ((i * (t[1] - t[0]) + j * (t[2] - t[0])) % 8 == 0).all()
                # the voxels p with 64p <= pt <= 64p + 64 per axis: floor(pt / 64), and the one below where pt is a multiple of 64
                ranges = [[q for q in ({int(c) // U, (int(c) - 1) // U} if c % U == 0 else {int(c) // U}) if 0 <= q < S] for c in pt]
                for x in ranges[0]:
                    for y in ranges[1]:
                        for z in ranges[2]:
                            assert sel[x, y, z], (t, pt)
                            checked += 1
    assert checked > 3000


def test_model_is_the_predicate_in_python_integers():
    S = 6
    rng = np.random.default_rng(3)
    grid = np.indices((S, S, S)).reshape(3, -1).T.tolist()
    for t in random_triangles(rng, S, 40):
        want = {tuple(p) for p in grid if model.touches_int(t, p)}
        assert as_set(model.touched_voxels(S, t)) == want, t
    # at the limits: the largest normal and dot products there are
    L = model.LIMIT
    for t in ([-L, -L, -L, L, L, L, L, -L, 0], [L, -L, 0, -L, L, 1, L, L, -1], [-L, L, U * S, L, -L, 0, L, L, 5]):
        want = {tuple(p) for p in grid if model.touches_int(t, p)}
        assert as_set(model.touched_voxels(S, t)) == want and len(want) > 0, t


# ---- 2. the pruning of the kernel against the predicate ---------------------------------------------------------------

LINE = re.compile(r"tri (\w+) S=(\d+) v=([-0-9,]+) covered=([01]) tested=(\d+) selected=(\d+) box=(\d+)")
CORNER = re.compile(r"corner S=512 tested=(\d+) selected=(\d+) box=(\d+)")
KINDS = ("general", "degenerate", "aligned", "boundary", "outside", "sliver", "lattice")
PER_KIND = 300


@pytest.fixture(scope="module")
def rule_report(tmp_path_factory):
    """what tests/cpp/raster_rule_main.cpp prints, built with the address and undefined-behaviour sanitizers and run as a program
    of its own"""
    exe = str(tmp_path_factory.mktemp("raster") / "raster_rule_main")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "raster_rule_main.cpp"), "-o", exe])
    return subprocess.run([exe, str(PER_KIND), "7"], capture_output=True, text=True, timeout=300)


def test_pruning_never_drops_a_voxel(rule_report):
    out = rule_report
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]      # a sanitizer report goes to stderr and ends the run
    lines = out.stdout.splitlines()
    rows = [m.groups() for m in map(LINE.fullmatch, lines) if m]
    assert len(rows) == len(lines) - 2 == 2 * len(KINDS) * PER_KIND and lines[-1] == "all_covered=1" and CORNER.fullmatch(lines[-2])
    assert all(r[3] == "1" for r in rows)
    assert {(r[0], r[1]) for r in rows} == {(k, s) for k in KINDS for s in ("8", "16")}
    # the program's predicate is the model's: voxel counts of a sample of its triangles
    for r in rows[::70]:
        assert int(r[5]) == len(model.touched_voxels(int(r[1]), [int(q) for q in r[2].split(",")])), r
    for kind in KINDS:
        mine = [r for r in rows if r[0] == kind]
        assert sum(int(r[5]) > 0 for r in mine) > len(mine) // 4, kind        # the seeded triangles are not mostly outside
        assert all(int(r[5]) <= int(r[4]) for r in mine)
    # the bounding box is not what is walked: general triangles in 16^3
    general = [r for r in rows if r[0] == "general" and r[1] == "16"]
    assert 3 * sum(int(r[4]) for r in general) < sum(int(r[6]) for r in general)


def test_corner_to_corner_cost(rule_report):
    """the figures quoted in include/vrc.h and csrc/vrc_raster.h for the triangle (0,0,0) (S,S,0) (S,0,S) of 512^3"""
    tested, selected, box = (int(q) for q in CORNER.fullmatch(rule_report.stdout.splitlines()[-2]).groups())
    print("corner to corner of 512^3: predicate applied to %d voxels, %d selected, bounding box %d" % (tested, selected, box))
    assert (tested, selected, box) == (524287, 524287, 512 ** 3)
    hdr = open(os.path.join(ROOT, "include", "vrc.h")).read()
    assert "524 287" in hdr and "134 217 728" in hdr
    # the same triangle at 32^3 through the model: the count scales as 2 S^2 - 1
    assert len(model.touched_voxels(32, model.corner_triangle(32)[0])) == 2 * 32 * 32 - 1


# ---- 3. refusals, symbols, constants, wrappers ------------------------------------------------------------------------

def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


VOLUME = handle(w2=5)                      # `depth` is the third 32-bit word of a vrc_volume
BUFFER = (C.c_int32 * 27)(*range(27))
MANY = 0x80000000                          # one more than a launch takes
NAME = "vrc_raster_mesh"


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


def args(v=VOLUME, n=3, tris=BUFFER, mode=0, solid=1, mem=0):
    return (p(v), n, p(tris), mode, solid, mem, None)


# every refusal of the entry point, all before the first HIP call: the WHOLE vrc_last_error() text, as literals
REFUSALS = [
    (args(v=None), "null volume"),
    (args(v=None, mode=1, mem=1), "null volume"),
    (args(mem=2), "bad mem kind 2"),
    (args(mem=-1, n=0), "bad mem kind -1"),
    (args(mode=2), "unknown mode 2"),
    (args(mode=-1, mem=1), "unknown mode -1"),
    (args(mode=7, n=0, tris=None), "unknown mode 7"),
    (args(tris=None), "null buffer"),
    (args(tris=None, mode=1, mem=1, solid=0), "null buffer"),
    (args(n=MANY), "too many triangles for one launch"),
    (args(n=1 << 40, mode=1, mem=1), "too many triangles for one launch"),
]


def untouched():
    return list(VOLUME) == [0, 0, 5] + [0] * 125 and list(BUFFER) == list(range(27))


@pytest.mark.parametrize("index", range(len(REFUSALS)))
def test_raster_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    call, text = REFUSALS[index]
    assert L.vrc_raster_mesh(*call) == -1                             # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (NAME, text)).encode()
    assert untouched()                                                       # nothing was written through the handle or the buffer


def test_nothing_to_do_is_ok_before_any_device_call(built):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    for mem in (0, 1):
        for mode in (capi.VRC_RASTER_TOUCHED, capi.VRC_RASTER_THIN):
            assert L.vrc_raster_mesh(*args(n=0, tris=None, mode=mode, mem=mem)) == 0
    assert untouched()


def test_symbol_and_constants():
    from cpuvoxelraycaster_amd import capi
    assert NAME in capi.SYMBOLS and len(capi.SYMBOLS[NAME][1]) == 7
    # a feature's entry points carry the feature's prefix (vrc_stroke_*, vrc_columns_*, ...): its refusals are listed here, not
    # in the closed table of test_volume_messages_host.py
    assert [n for n in capi.SYMBOLS if n.startswith("vrc_raster_")] == [NAME]
    assert (capi.VRC_RASTER_TOUCHED, capi.VRC_RASTER_THIN) == (model.TOUCHED, model.THIN) == (0, 1)
    hdr = os.path.join(ROOT, "include", "vrc.h")
    check_cpp_syntax('#include "%s"\nstatic_assert(VRC_RASTER_TOUCHED == 0 && VRC_RASTER_THIN == 1, "modes");\nint main() { return 0; }\n' % hdr,
                     strict=True)


def test_wrappers_exist():
    import cpuvoxelraycaster_amd as vrc
    for name in ("rasterMesh", "shellMesh", "solidFromShell"):
        assert callable(getattr(vrc.VoxelVolume, name)), name


def test_host_adapter_with_raster_compiles():
    """HipVoxelVolume::rasterMesh / rasterMeshDevice / shellMesh in the header-only adapter: C++14, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'void use(vrc_host::HipVoxelVolume& world, const std::vector<int32_t>& tris, const std::vector<double>& verts,\n'
           '         const std::vector<uint32_t>& faces) {\n'
           '    world.rasterMesh(tris);\n'
           '    world.rasterMesh(tris, VRC_RASTER_THIN, false);\n'
           '    world.rasterMeshDevice(tris.size() / 9, tris.data(), VRC_RASTER_TOUCHED, true, nullptr);\n'
           '    world.shellMesh(verts, faces);\n'
           '    world.shellMesh(verts, faces, true, false, 2.0, 1.0, 2.0, 3.0);\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)


def test_kernel_header_runs_on_the_host_without_hip():
    """csrc/vrc_raster.h is free of HIP types: a plain C++14 compiler takes it"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "csrc", "vrc_raster.h")
    check_cpp_syntax('#include "%s"\nint main() { int64_t n[3]; const int64_t v[9] = {0, 0, 0, 64, 0, 0, 0, 64, 0};\n'
                     '    vrc::raster_normal(v, n); return n[2] == 4096 ? 0 : 1; }\n' % hdr, strict=True)
