"""The capsule brush without a GPU: the numpy model (stroke_model.py) against the rule in Python integers and against its own
identities, the piece boxes of csrc/vrc_stroke.h held to the rule by brute force in a sanitized stand-alone program, every
refusal that precedes a device call by its whole text, the symbols, the constant and the C++ adapter's new methods."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import large_volume_cases as cases
import stroke_model as model
from volume_support import ROOT, check_cpp_syntax

LIMIT = 8192


def random_items(rng, S, count, far=False):
    """capsules around a volume of S^3: ends a little outside, some degenerate, some axis-aligned, radius -1 .. 6"""
    a = rng.integers(-6, S + 6, (count, 3))
    b = rng.integers(-6, S + 6, (count, 3))
    kind = rng.integers(0, 6, count)
    b[kind == 0] = a[kind == 0]
    for axis in range(3):
        same = (kind == 1) & (rng.integers(0, 3, count) != axis)
        b[same, axis] = a[same, axis]
    if far:
        a[kind == 2, 0] = -rng.integers(0, LIMIT + 1, int((kind == 2).sum()))
        b[kind == 2, 2] = rng.integers(0, LIMIT + 1, int((kind == 2).sum()))
    r = rng.integers(-1, 7, (count, 1))
    return np.concatenate([a, b, r, np.zeros((count, 1), np.int64)], axis=1).astype(np.int32)


# ---- 1. the model against big integers -------------------------------------------------------------------------------

def test_model_is_the_rule_in_python_integers():
    S = 16
    rng = np.random.default_rng(16)
    grid = np.indices((S, S, S)).reshape(3, -1).T
    for item in random_items(rng, S, 300).tolist():
        want = np.array([model.rule_int(p, item) for p in grid.tolist()], bool).reshape(S, S, S)
        got = np.zeros((S, S, S), np.uint8)
        model.fill_capsules(got, [item], 1)
        assert np.array_equal(got.astype(bool), want), item
        sparse = model.capsule_voxels_sparse(S, item)
        assert sorted(map(tuple, sparse.tolist())) == sorted(map(tuple, np.argwhere(want).tolist())), item


def test_model_does_not_overflow_at_the_limits():
    """int64 at the corner voxels of 1024^3 for items whose coordinates and radius are +-8192: the largest q, d and r there are"""
    S = 1024
    corners = np.array([(x, y, z) for x in (0, S - 1) for y in (0, S - 1) for z in (0, S - 1)], np.int64)
    ends = [(x, y, z) for x in (-LIMIT, LIMIT) for y in (-LIMIT, LIMIT) for z in (-LIMIT, LIMIT)]
    checked = inside = 0
    for a in ends:
        for b in ends:
            for r in (0, 1, LIMIT - 1, LIMIT):
                item = list(a) + list(b) + [r, 0]
                got = model.rule(corners[:, 0], corners[:, 1], corners[:, 2], item)
                want = [model.rule_int(p, item) for p in corners.tolist()]
                assert got.tolist() == want, item
                checked += len(want)
                inside += sum(want)
    assert checked == 8 * 8 * 4 * 8 and 0 < inside < checked
    # and between the ends, where the third case's products are largest: a long diagonal that passes the volume
    for item in ([-LIMIT, -LIMIT, -LIMIT, LIMIT, LIMIT, LIMIT, 700, 0], [-LIMIT, LIMIT, -LIMIT, LIMIT, -LIMIT + 1023, LIMIT, 1023, 0],
                 [LIMIT, LIMIT, -LIMIT, -LIMIT, -LIMIT, LIMIT, LIMIT, 0]):
        got = model.rule(corners[:, 0], corners[:, 1], corners[:, 2], item)
        assert got.tolist() == [model.rule_int(p, item) for p in corners.tolist()], item


# ---- 2. the model's identities ---------------------------------------------------------------------------------------

def test_degenerate_capsule_is_the_sphere():
    S = 32
    rng = np.random.default_rng(2)
    for cx, cy, cz, r in np.concatenate([rng.integers(-5, S + 5, (60, 3)), rng.integers(-1, 12, (60, 1))], axis=1).tolist():
        a, b = np.zeros((S, S, S), np.uint8), np.zeros((S, S, S), np.uint8)
        model.fill_capsules(a, [[cx, cy, cz, cx, cy, cz, r, 0]], 1)
        cases.fill_spheres(b, [[cx, cy, cz, r]], 1)
        assert np.array_equal(a, b), (cx, cy, cz, r)


def test_swapping_the_ends_changes_nothing():
    S = 24
    for item in random_items(np.random.default_rng(3), S, 200, far=True).tolist():
        swapped = item[3:6] + item[0:3] + item[6:]
        a, b = model.capsule_voxels(S, item), model.capsule_voxels(S, swapped)
        assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist())), item


def test_capsule_contains_the_balls_along_its_segment():
    S = 32
    rng = np.random.default_rng(4)
    for item in random_items(rng, S, 120).tolist():
        if item[6] < 0:
            assert len(model.capsule_voxels(S, item)) == 0
            continue
        vol = np.zeros((S, S, S), np.uint8)
        model.fill_capsules(vol, [item], 1)
        a, b = np.array(item[0:3]), np.array(item[3:6])
        g = int(np.gcd.reduce(np.abs(b - a))) or 1
        lattice = [a + (b - a) // g * k for k in range(g + 1)]               # every lattice point of the segment, the ends first and last
        balls = np.zeros_like(vol)
        cases.fill_spheres(balls, [list(p) + [item[6]] for p in lattice], 1)
        assert not (balls & ~vol).any(), item
        if item[6] == 0:                                                    # r == 0: exactly the lattice points
            assert np.array_equal(balls, vol), item


def test_dropped_items():
    S = 16
    m = S // 2
    assert len(model.capsule_voxels(S, [m, m, m, m + 3, m, m, 1, 0])) > 0
    for dropped in ([LIMIT + 1, m, m, m, m, m, LIMIT, 0], [m, -LIMIT - 1, m, m, m, m, LIMIT, 0], [m, m, m, m, m, LIMIT + 1, LIMIT, 0],
                    [m, m, m, m, m, -LIMIT - 1, LIMIT, 0], [m, m, m, m, m, m, LIMIT + 1, 0], [m, m, m, m + 3, m, m, 1, 1],
                    [m, m, m, m + 3, m, m, 1, -1], [m, m, m, m + 3, m, m, -1, 0], [m, m, m, m, m, m, -LIMIT - 5, 0]):
        assert len(model.capsule_voxels(S, dropped)) == 0 and len(model.capsule_voxels_sparse(S, dropped)) == 0, dropped
    for kept in ([LIMIT, m, m, m, m, m, LIMIT, 0], [m, m, -LIMIT, m, m, m, LIMIT, 0], [m, m, m, m, m, m, LIMIT, 0]):
        assert len(model.capsule_voxels(S, kept)) == S ** 3, kept             # the largest values kept reach everything
    vol = np.ones((S, S, S), np.uint8)
    model.fill_capsules(vol, [[m, m, m, m, m, m, LIMIT + 1, 0], [0, 0, 0, S, S, S, 0, 0]], 0)
    assert int(vol.sum()) == S ** 3 - S                                       # the first is dropped, the second is the diagonal's S voxels


def test_stroke_items():
    c = np.array([(1, 1, 1), (4, 1, 1), (0, 0, 0), (9, 9, 9), (9, 9, 12), (20, 9, 12)])
    valid = np.array([1, 1, 0, 1, 1, 1], bool)
    assert model.stroke_items(c, valid, 2, 0).tolist() == [[1, 1, 1, 4, 1, 1, 2, 0], [4, 1, 1, 4, 1, 1, 2, 0], [9, 9, 9, 9, 9, 12, 2, 0],
                                                            [9, 9, 12, 20, 9, 12, 2, 0], [20, 9, 12, 20, 9, 12, 2, 0]]
    assert model.stroke_items(c, valid, 0, 3).tolist() == [[1, 1, 1, 4, 1, 1, 0, 0], [4, 1, 1, 4, 1, 1, 0, 0], [9, 9, 9, 9, 9, 12, 0, 0],
                                                            [9, 9, 12, 9, 9, 12, 0, 0], [20, 9, 12, 20, 9, 12, 0, 0]]
    assert model.stroke_items(c, valid, 1, 2)[:, 3:6].tolist() == [[1, 1, 1], [4, 1, 1], [9, 9, 9], [9, 9, 12], [20, 9, 12]]
    assert model.stroke_items(c[:0], valid[:0], 1, 0).shape == (0, 8)


# ---- 3. the piece boxes ----------------------------------------------------------------------------------------------

LINE = re.compile(r"(seeded|limits|thin|sums) (\d+) S=(\d+) item=([-0-9,]+) covered=([01]) voxels=(\d+) pieces=(\d+) piece_items=(\d+) box_items=(\d+)")


@pytest.fixture(scope="module")
def pieces_report(tmp_path_factory):
    """what tests/cpp/stroke_pieces_main.cpp prints, built with the address and undefined-behaviour sanitizers and run as a
    program of its own"""
    exe = str(tmp_path_factory.mktemp("stroke") / "stroke_pieces_main")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "stroke_pieces_main.cpp"), "-o", exe])
    out = subprocess.run([exe, "3000", "7"], capture_output=True, text=True, timeout=300)
    return out


def test_piece_boxes_cover_the_rule(pieces_report):
    out = pieces_report
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]      # a sanitizer report goes to stderr and ends the run
    assert "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout
    rows = [m.groups() for m in map(LINE.fullmatch, out.stdout.splitlines()) if m]
    assert len(rows) == len(out.stdout.splitlines()) - 1 and out.stdout.splitlines()[-1] == "all_covered=1"
    by_set = {s: [r for r in rows if r[0] == s] for s in ("seeded", "limits", "thin", "sums")}
    assert [len(by_set[s]) for s in ("seeded", "limits", "thin", "sums")] == [3000, 13, 18, 2]
    assert all(r[4] == "1" for r in rows)                                     # covered, every capsule
    # the program's rule is the model's: voxel counts of a sample of its capsules
    for r in by_set["seeded"][::60] + by_set["limits"] + by_set["thin"][:3]:
        item = [int(v) for v in r[3].split(",")]
        count = len(model.capsule_voxels_sparse(int(r[2]), item) if r[0] == "thin" else model.capsule_voxels(int(r[2]), item))
        assert int(r[5]) == count, r
    assert sum(int(r[5]) > 0 for r in by_set["seeded"]) > 1500                # the seeded capsules are not mostly empty
    assert [int(r[5]) for r in by_set["limits"][-3:]] == [0, 0, 0]           # the three dropped items
    assert [int(by_set["limits"][i][5]) for i in (4, 6, 7)] == [64 ** 3] * 3  # radius 8192 around a centre or a segment that meets the volume
    # the named thin cases at 256^3 are there, each at r = 0, 1, 3
    thin = {(tuple(int(v) for v in r[3].split(",")[:6]), int(r[3].split(",")[6])) for r in by_set["thin"]}
    for ends in ((-40, -40, -40, 295, 295, 295), (0, 0, 0, 255, 1, 0), (0, 3, 250, 255, 254, 253)):
        assert all((ends, rad) in thin for rad in (0, 1, 3))
    print("\n".join(" ".join(r) for r in by_set["thin"] + by_set["sums"]))


def test_a_thin_diagonal_is_cut_up(pieces_report):
    """the whole diagonal of 512^3 with r = 3: the pieces' word items against those of the capsule's bounding box, which is the
    whole volume.  Measured: 17504 of 4259840, 1/243; the bound only says that the capsule is cut up at all"""
    rows = [m.groups() for m in map(LINE.fullmatch, pieces_report.stdout.splitlines()) if m and m.group(1) == "sums"]
    diagonal = rows[0]
    assert diagonal[3] == "0,0,0,511,511,511,3,0" and diagonal[2] == "512"
    piece_items, box_items = int(diagonal[7]), int(diagonal[8])
    print("diagonal of 512^3, r = 3: piece word items %d, bounding-box word items %d, ratio 1/%.0f" % (piece_items, box_items, box_items / piece_items))
    assert box_items == cases.whole_box_items(9)
    assert 0 < piece_items * 16 < box_items


# ---- 4. refusals, symbols, the constant, the adapter ------------------------------------------------------------------

def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


VOLUME = handle(w2=5)                      # `depth` is the third 32-bit word of a vrc_volume
BUFFER = (C.c_int32 * 24)(*range(24))
MANY = 0x80000000                          # one more than a launch takes


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


def capsules_args(v=VOLUME, n=2, items=BUFFER, solid=1, mem=0):
    return (p(v), n, p(items), solid, mem, None)


def hits_args(v=VOLUME, n=2, hits=BUFFER, radius=2, max_gap=0, solid=1, mem=0):
    return (p(v), n, p(hits), radius, max_gap, solid, mem, None)


# every refusal of the vrc_stroke_* entry points, all before the first HIP call: the WHOLE vrc_last_error() text, as literals
REFUSALS = [
    ("vrc_stroke_fill_capsules", capsules_args(v=None), "null volume"),
    ("vrc_stroke_fill_capsules", capsules_args(mem=2), "bad mem kind 2"),
    ("vrc_stroke_fill_capsules", capsules_args(mem=-1, n=0), "bad mem kind -1"),
    ("vrc_stroke_fill_capsules", capsules_args(items=None), "null buffer"),
    ("vrc_stroke_fill_capsules", capsules_args(items=None, mem=1), "null buffer"),
    ("vrc_stroke_fill_capsules", capsules_args(n=MANY), "too many capsules for one launch"),
    ("vrc_stroke_fill_capsules", capsules_args(n=1 << 40, mem=1), "too many capsules for one launch"),
    ("vrc_stroke_fill_at_hits", hits_args(v=None), "null volume"),
    ("vrc_stroke_fill_at_hits", hits_args(mem=7), "bad mem kind 7"),
    ("vrc_stroke_fill_at_hits", hits_args(mem=-1, n=0), "bad mem kind -1"),
    ("vrc_stroke_fill_at_hits", hits_args(radius=-1), "radius -1 not in [0, 2^13]"),
    ("vrc_stroke_fill_at_hits", hits_args(radius=8193, n=0), "radius 8193 not in [0, 2^13]"),
    ("vrc_stroke_fill_at_hits", hits_args(radius=1 << 20, mem=1), "radius 1048576 not in [0, 2^13]"),
    ("vrc_stroke_fill_at_hits", hits_args(hits=None), "null buffer"),
    ("vrc_stroke_fill_at_hits", hits_args(hits=None, mem=1, max_gap=4), "null buffer"),
    ("vrc_stroke_fill_at_hits", hits_args(n=MANY), "too many hits for one launch"),
    ("vrc_stroke_fill_at_hits", hits_args(n=MANY, radius=8192, mem=1), "too many hits for one launch"),
]


def untouched():
    return list(VOLUME) == [0, 0, 5] + [0] * 125 and list(BUFFER) == list(range(24))


@pytest.mark.parametrize("index", range(len(REFUSALS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(REFUSALS)])
def test_stroke_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    name, args, text = REFUSALS[index]
    assert getattr(L, name)(*args) == -1                                     # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
    assert untouched()                                                       # nothing was written through the handle or the buffer


def test_nothing_to_do_is_ok_before_any_device_call(built):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    for mem in (0, 1):
        assert L.vrc_stroke_fill_capsules(*capsules_args(n=0, items=None, mem=mem)) == 0
        assert L.vrc_stroke_fill_at_hits(*hits_args(n=0, hits=None, mem=mem, radius=8192)) == 0
    assert untouched()


def test_every_stroke_entry_point_has_its_refusals():
    from cpuvoxelraycaster_amd import capi
    names = {n for n in capi.SYMBOLS if n.startswith("vrc_stroke_")}
    assert names == {"vrc_stroke_fill_capsules", "vrc_stroke_fill_at_hits"} == {c[0] for c in REFUSALS}
    assert not any(n.startswith(("vrc_volume_", "vrc_labels_", "vrc_distance_")) or "pack_" in n for n in names)
    assert capi.VRC_STROKE_LIMIT == model.LIMIT == LIMIT


def test_the_limit_is_public():
    hdr = os.path.join(ROOT, "include", "vrc.h")
    check_cpp_syntax('#include "%s"\nstatic_assert(VRC_STROKE_LIMIT == 8192, "2^13");\nint main() { return 0; }\n' % hdr, strict=True)


def test_wrappers_exist():
    import cpuvoxelraycaster_amd as vrc
    for name in ("fillCapsules", "fillCapsulesDevice", "strokeAtHits", "strokeAtHitsDevice", "fillLine", "fillPolyline"):
        assert callable(getattr(vrc.VoxelVolume, name)), name


def test_host_adapter_with_strokes_compiles():
    """HipVoxelVolume::fillCapsules / fillCapsulesDevice / fillLine / fillPolyline / strokeAtHits / strokeAtHitsDevice in the
    header-only adapter: C++14, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'void use(vrc_host::HipVoxelVolume& world, const std::vector<vrc_hit>& hits) {\n'
           '    const int32_t a[3] = {1, 2, 3}, b[3] = {40, -5, 9};\n'
           '    std::vector<vrc_host::HipVoxelVolume::Capsule> items(2);\n'
           '    world.fillCapsules(items, true);\n'
           '    world.fillCapsulesDevice(2, &items[0].ax, false, nullptr);\n'
           '    world.fillLine(a, b, 2, true);\n'
           '    world.fillPolyline(std::vector<int32_t>(9, 4), 1, false, true);\n'
           '    world.strokeAtHits(hits, 3, false);\n'
           '    world.strokeAtHits(hits, 3, true, 12u);\n'
           '    world.strokeAtHitsDevice(hits.size(), hits.data(), 0, false, 4u, nullptr);\n'
           '    static_assert(sizeof(vrc_host::HipVoxelVolume::Capsule) == 32, "n x 8 int32");\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
