"""The cases of tests/test_gpu_volume_morph_large.py: elements and sources at which k_morph_apply (csrc/vrc_morph.hip) leaves
the regime the smaller tests keep it in.  Three things, numpy only:
  the kernel's geometry restated from the code as it stands, each with the line it was read off, so that the host test
      (tests/test_morph_cases_host.py) can hold the cases to the tiles, blocks, pitches and byte ranges they are meant for;
  dense cases: an element and a source TUNED to it -- the set being ORed gets the density at which the OR of the element's
      n samples is solid with probability one half, so that every offset decides voxels and a lost column, mask bit or
      pillar shows.  morph_model.source() saturates from about thirty offsets upwards (the table in the host test's
      docstring);
  sparse cases for 512^3 and 1024^3 as lists of coordinates, never an S^3 array, with the expected sets as lists."""
import functools

import numpy as np

import cells_model
import morph_model as model
from levels_cases import in_list_order  # noqa: F401  (the order of VoxelVolume.voxels(), restated once)

DILATE, ERODE, SOLID, EMPTY, REACH = model.DILATE, model.ERODE, model.SOLID, model.EMPTY, model.REACH
COMBOS = [(what, of, outside) for what in (DILATE, ERODE) for of in (SOLID, EMPTY) for outside in (0, 1)]


# ---- the geometry of k_morph_apply --------------------------------------------------------------------------------------

TILE = 16                            # vrc_morph.hip:46  constexpr uint32_t TILE = 16u: brick columns per axis of a workgroup's tile
SPAN = 2 * TILE                      # vrc_morph.hip:141 blockIdx * 2u * TILE: 32 voxel columns, and 32 voxels of z (:204, 4 words)


def tiles(S):
    """vrc_morph.hip:233  tiles = S > 2u * TILE ? S / (2u * TILE) : 1u; the grid is tiles^3 (:237)"""
    return S // SPAN if S > SPAN else 1


def interior_tiles(S):
    """the tile numbers of one axis whose reach-16 neighbourhood lies inside the volume: the staging test of :152 (cx < 0,
    cx >= n) is false for every brick column of the largest region [32 t - 16, 32 t + 48)"""
    return [t for t in range(tiles(S)) if SPAN * t - REACH >= 0 and SPAN * t + SPAN + REACH <= S]


def interior_z_blocks(S):
    """the blockIdx.z whose eight words 4 blockIdx.z - 2 + k (:158) all lie in [0, nz), nz = S / 8 (:132): the test of :160
    is true for every k"""
    nz = S // 8
    return [b for b in range(tiles(S)) if 4 * b - 2 >= 0 and 4 * b + 5 < nz]


def effective(e, what):
    """E' of the header comment (:8-10): E for DILATE and -E for ERODE, the distinct offsets as (n, 3) int64"""
    e = model.element(e)
    return e if what == DILATE else -e


def staged(e, what):
    """(LX, LY, pitch): :140  LX = 2 TILE + ax1 - ax0, LY = 2 TILE + ay1 - ay0 and :142  pitch = LY <= 48 ? 24 : 40"""
    ee = effective(e, what)
    LX, LY = SPAN + int(ee[:, 0].max() - ee[:, 0].min()), SPAN + int(ee[:, 1].max() - ee[:, 1].min())
    return LX, LY, 24 if LY <= 48 else 40


def byte_range(e, what):
    """(k_lo, k_hi): :148  k_lo = (REACH - az1) >> 3, k_hi = (47 - az0) >> 3, the bytes of a pillar that are staged"""
    ee = effective(e, what)
    return (REACH - int(ee[:, 2].max())) >> 3, (47 - int(ee[:, 2].min())) >> 3


def columns(e):
    """the length of the column list (:85): the distinct (ex, ey)"""
    return len(np.unique(model.element(e)[:, :2], axis=0))


def mask_bits(e):
    """the most bits in one z mask (:67)"""
    return int(np.unique(model.element(e)[:, :2], axis=0, return_counts=True)[1].max())


def tile_of(p):
    """(tile along x, tile along y, z block) of voxels (n, 3)"""
    return np.asarray(p, np.int64) // SPAN


def tile_fractions(k):
    """the solid fraction of every 32^3 tile of a dense result, [tx, ty, tz]; S >= 32"""
    T = k.shape[0] // SPAN
    return k.reshape(T, SPAN, T, SPAN, T, SPAN).mean(axis=(1, 3, 5))


def interior_fractions(k):
    """the fractions of the tiles that are interior in x, y and z, flat; empty below 128^3"""
    t = interior_tiles(k.shape[0])
    return tile_fractions(k)[np.ix_(t, t, t)].reshape(-1) if t else np.zeros(0)


# ---- elements -----------------------------------------------------------------------------------------------------------

PIECE_PIVOT = (5, 4, 6)


def piece_shape():
    """a 16^3 piece of several parts: its voxel list about PIECE_PIVOT is an element"""
    shape = np.zeros((16, 16, 16), np.uint8)
    shape[3:8, 4, 2:11] = shape[5, 4:9, 6] = shape[7, 7, 7] = shape[1, 1, 15] = 1
    shape[12, 9:14, 3] = shape[0, 15, 0] = 1
    return shape


def spread(rng, n, lo, hi):
    """n distinct offsets with component a in [lo[a], hi[a]], every bound met by one of them"""
    lo, hi = np.array(lo), np.array(hi)
    rows = {tuple(v) for v in (lo, hi)}
    while len(rows) < n:
        rows.add(tuple(rng.integers(lo, hi + 1).tolist()))
    return np.array(sorted(rows), np.int32)


@functools.lru_cache(maxsize=None)
def elements():
    """name -> (n, 3) int32, distinct offsets.  Shared: do not write to them."""
    rng = np.random.default_rng(1616)
    out = {"ball%d" % r: model.ball(r) for r in range(2, 7)}
    out.update(box3=model.box(3, 3, 3), box9=model.box(9, 9, 9), slab33=model.box(33, 1, 33, (16, 5, 16)))
    out.update({"line%d" % axis: model.line(axis, -16, 16) for axis in range(3)})
    for n in (48, 200, 400):                                                    # 400: more than 256 columns
        out["random%d" % n] = spread(rng, n, (-16, -16, -16), (16, 16, 16))
    out["one_sided"] = spread(rng, 60, (-16, -4, 9), (-9, 4, 16))              # DILATE: k_hi = 4; ERODE: k_lo = 3
    out["one_sided_reflected"] = model.reflect(out["one_sided"])                # DILATE: k_lo = 3; ERODE: k_hi = 4
    out["wy16"] = spread(rng, 40, (-5, -8, -6), (5, 8, 6))                     # LY = 48: pitch 24
    out["wy17"] = spread(rng, 40, (-5, -8, -6), (5, 9, 6))                     # LY = 49: pitch 40
    out["lx64"] = spread(rng, 40, (-16, -3, -16), (16, 3, 16))
    out["lx33"] = spread(rng, 40, (3, -7, -9), (4, 7, 9))
    out["piece"] = (np.argwhere(piece_shape()) - np.array(PIECE_PIVOT)).astype(np.int32)
    for e in out.values():
        assert len(model.element(e)) == len(e)
        e.setflags(write=False)
    return out


NAMES = ["ball2", "ball3", "ball4", "ball5", "ball6", "box3", "box9", "slab33", "line0", "line1", "line2", "random48", "random200", "random400",
         "one_sided", "one_sided_reflected", "wy16", "wy17", "lx64", "lx33", "piece"]
SIZES = [32, 64, 128, 256]
SAMPLED = ("random200", "random400", "ball6")       # "every offset matters" on 16 offsets, the extreme ones among them


def forms_of(name, S):
    """all eight below 256^3; there two that differ in `what` and `outside`, one of each source, another pair from element to element"""
    i = NAMES.index(name)
    return COMBOS if S < 256 else [COMBOS[i % 8], COMBOS[(i % 8) ^ 5]]


def density_of(n):
    """the density of the set being ORed at which the OR of n independent samples is solid with probability one half"""
    return 1.0 - 0.5 ** (1.0 / n)


def ored_is_sparse_solid(what, of):
    """the solid voxels are the set being ORed (density d) when this holds, its complement (1 - d) otherwise"""
    return (of == SOLID) == (what == DILATE)


# At 256^3 there are 216 interior tiles, and an element of 500 offsets and more leaves few independent samples in each: the
# least or the greatest of them leaves [0.35, 0.65] for most seeds.  These are the first seeds from 6000 on for which the
# model's result stays within 0.148 of one half in every interior tile for both forms (ball6: the first from 7000 on in steps
# of 400 seeds searched side by side).  Searched on the model alone.
CHOSEN_SEEDS = {("ball5", 256): 6000, ("box9", 256): 6002, ("slab33", 256): 6007, ("ball6", 256): 8222}


def seed_of(name, S):
    return CHOSEN_SEEDS.get((name, S), 1000 * SIZES.index(S) + NAMES.index(name))


def source_for(n, seed, S, sparse=True):
    """dense [x, y, z] uint8: fillRandom's set of `seed` at the density tuned to an element of n distinct offsets, or at one
    minus it.  Do not write to it."""
    d = density_of(n)
    vol = cells_model.random_set(seed, cells_model.threshold_of(d if sparse else 1.0 - d), S)
    vol.setflags(write=False)
    return vol


def tuned_source(name, S, sparse):
    """source_for the named element at its seed"""
    return source_for(len(elements()[name]), seed_of(name, S), S, sparse)


def faces_read_solid(what, outside):
    """`edge` of morph_run (:231): beyond the faces the ORed set reads as present.  Then the result at p is one constant,
    whatever the source holds, wherever some p - e' (e' of the effective element) lies beyond a face; the interior tiles
    see no face."""
    return (outside != 0) != (what == ERODE)


def forced_fractions(e, what, S):
    """per 32^3 tile, the fraction of its voxels at which a form with faces_read_solid gives that constant: the voxels p with
    some p - e' outside the volume, which is the model's dilation of an EMPTY volume by the effective element with
    everything beyond the faces present.  No source enters."""
    return tile_fractions(model.morph_words(np.zeros((S, S, S), np.uint8), DILATE, effective(e, what), SOLID, 1))


def tile_bound_is_impossible(e, what, outside, S):
    """the host test's every-tile bound [0.03, 0.97] cannot be met by any source: faces read solid and some tile has more
    than 97 % of its voxels forced.  For a line of -16 .. 16 at 32^3 that is every voxel of the one tile."""
    return faces_read_solid(what, outside) and bool(forced_fractions(e, what, S).max() > 0.97)


# ---- sparse cases for 512^3 and 1024^3 -----------------------------------------------------------------------------------

LARGE_ELEMENTS = ["ball3", "line0", "line1", "line2"]


@functools.lru_cache(maxsize=None)
def sparse_tiles(S):
    """(80, 3): the 64 tiles with numbers 0, 1, T / 2 and T - 1 on every axis, and 16 seeded others"""
    T = tiles(S)
    chosen = [(x, y, z) for x in (0, 1, T // 2, T - 1) for y in (0, 1, T // 2, T - 1) for z in (0, 1, T // 2, T - 1)]
    rng = np.random.default_rng(S)
    while len(chosen) < 80:
        t = tuple(rng.integers(0, T, 3).tolist())
        if t not in chosen:
            chosen.append(t)
    return np.array(chosen, np.int64)


def local_arrangement(i):
    """the voxels of the i-th chosen tile, local coordinates (m, 3): three pairs on the seams (31 on one side, 0 on the
    other), one at the tile's far corner for every second tile, and 24 + i % 9 seeded ones -- another set in every tile"""
    rng = np.random.default_rng(7000 + i)
    a, b, c = (int(v) for v in rng.integers(0, SPAN, 3))
    seams = [(31, a, b), (0, a, (b + i) % SPAN), (c, 31, a), (b, 0, c), (a, c, 31), (c, (a + i) % SPAN, 0)]
    corner = [(31, 31, 31)] if i % 2 == 0 else [(0, 31, 0)]
    return np.unique(np.array(seams + corner + rng.integers(0, SPAN, (24 + i % 9, 3)).tolist(), np.int64), axis=0)


@functools.lru_cache(maxsize=None)
def sparse_points(S):
    """(n, 3) int64, distinct, in the order of the voxel list: the solid voxels of the DILATE source and the holes of the
    ERODE one.  Shared: do not write to it."""
    parts = [SPAN * t + local_arrangement(i) for i, t in enumerate(sparse_tiles(S))]
    m = S // 2 + 5
    faces = [(0, m, 77), (S - 1, 78, m), (m, 0, 79), (80, S - 1, m), (m, 81, 0), (82, m, S - 1), (S - 1, S - 1, S - 1), (0, 0, 0)]
    p = in_list_order(np.concatenate(parts + [np.array(faces, np.int64)]), S.bit_length() - 1)
    p.setflags(write=False)
    return p


def dilated(points, e, S):
    """the distinct {p + e} inside the volume, in list order: the dilation of the solid set `points`, outside = 0"""
    q = (np.asarray(points, np.int64)[:, None, :] + model.element(e)[None, :, :]).reshape(-1, 3)
    return in_list_order(q[((q >= 0) & (q < S)).all(axis=1)], S.bit_length() - 1)


def erosion_holes(holes, e, S):
    """the distinct {h - e} inside the volume: what the erosion (outside = 1) of the full volume without `holes` leaves empty"""
    return dilated(holes, model.reflect(model.element(e)), S)


# ---- the list at its cap ---------------------------------------------------------------------------------------------------

MAX_OFFSETS = 1 << 20                # include/vrc.h: VRC_MORPH_MAX_OFFSETS


@functools.lru_cache(maxsize=None)
def capped_list():
    """(the 100 distinct offsets, the same repeated to 1 048 576 rows and shuffled).  Shared: do not write to them."""
    rng = np.random.default_rng(100)
    e = spread(rng, 100, (-16, -16, -16), (16, 16, 16))
    rows = np.resize(e, (MAX_OFFSETS, 3)).copy()
    rng.shuffle(rows)
    for a in (e, rows):
        a.setflags(write=False)
    return e, rows
