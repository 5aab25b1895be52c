"""The numpy model of vrc_morph_apply (include/vrc.h): the yardstick of test_volume_morph_host.py, test_gpu_volume_morph.py,
test_gpu_volume_morph_cpp.py and, with the cases of morph_cases.py, test_gpu_volume_morph_large.py.  Occupancy is dense
[x, y, z] uint8.  The set A is padded by the reach with `outside`, and K is the OR (dilate) or AND (erode) of one shifted
slice per distinct offset.  The element helpers are the twins of the package's."""
import numpy as np

from cells_model import apply_op, random_set, three_band, threshold_of     # noqa: F401  (the tests' sources)

REPLACE, OR, ANDNOT = 0, 1, 2
DILATE, ERODE = 0, 1
SOLID, EMPTY = 1, 2
REACH = 16


def element(offsets, origin=None):
    """the distinct offsets minus the origin as a sorted (n, 3) int64 array"""
    e = np.asarray(offsets, np.int64).reshape(-1, 3)
    if origin is not None:
        e = e - np.asarray(origin, np.int64).reshape(1, 3)
    return np.unique(e, axis=0) if len(e) else e


def in_reach(offsets):
    """the offsets a device-memory call keeps: every component within the reach"""
    e = np.asarray(offsets, np.int64).reshape(-1, 3)
    return e[(np.abs(e) <= REACH).all(axis=1)]


def morph(vol, what, offsets, of=SOLID, outside=0, origin=None):
    """K as uint8 [x, y, z]"""
    S = vol.shape[0]
    a = (np.asarray(vol) != 0) if of == SOLID else (np.asarray(vol) == 0)
    padded = np.pad(a, REACH, constant_values=bool(outside))
    k = np.zeros((S, S, S), bool) if what == DILATE else np.ones((S, S, S), bool)
    sign = -1 if what == DILATE else 1                        # dilate reads p - e, erode p + e
    for ex, ey, ez in element(offsets, origin).tolist():
        assert max(abs(ex), abs(ey), abs(ez)) <= REACH
        x, y, z = REACH + sign * ex, REACH + sign * ey, REACH + sign * ez
        part = padded[x:x + S, y:y + S, z:z + S]
        k = (k | part) if what == DILATE else (k & part)
    return k.astype(np.uint8)


def morph_words(vol, what, offsets, of=SOLID, outside=0, origin=None):
    """morph() for S >= 64 with the 64 voxels of a z run in one uint64: the same padding, the same slice per offset, one eighth
    of the memory a pass moves.  The z shift is made on the bytes before they are packed (once per distinct ez), so no bit
    moves between words here.  test_morph_cases_host.py holds it to morph() on every element of morph_cases.py at 64^3
    and on six of them at 128^3."""
    S = vol.shape[0]
    if S < 64:
        return morph(vol, what, offsets, of, outside, origin)
    a = (np.asarray(vol) != 0) if of == SOLID else (np.asarray(vol) == 0)
    padded = np.pad(a, REACH, constant_values=bool(outside))
    k = np.zeros((S, S, S // 64), np.uint64) if what == DILATE else np.full((S, S, S // 64), ~np.uint64(0))
    sign = -1 if what == DILATE else 1
    e = element(offsets, origin)
    assert not len(e) or np.abs(e).max() <= REACH
    for ez in np.unique(e[:, 2]).tolist() if len(e) else []:
        z = REACH + sign * ez
        plane = np.packbits(padded[:, :, z:z + S], axis=2).view(np.uint64)         # (S + 32, S + 32, S / 64)
        for ex, ey in e[e[:, 2] == ez][:, :2].tolist():
            x, y = REACH + sign * ex, REACH + sign * ey
            if what == DILATE:
                k |= plane[x:x + S, y:y + S]
            else:
                k &= plane[x:x + S, y:y + S]
    return np.unpackbits(k.view(np.uint8), axis=2)


def apply(dst, vol, what, offsets, of=SOLID, outside=0, op=REPLACE, origin=None):
    """dst after the call"""
    return apply_op(np.asarray(dst, np.uint8), morph(vol, what, offsets, of, outside, origin), op)


def fits_at(vol, offsets):
    return morph(vol, ERODE, offsets, EMPTY, 0)


def match(vol, solid_offsets, empty_offsets, outside=0):
    k = morph(vol, ERODE, solid_offsets, SOLID, outside)
    return apply_op(k, morph(vol, DILATE, reflect(empty_offsets), SOLID, outside), ANDNOT)


# ---- the element helpers' twins ------------------------------------------------------------------------------------

def ball(r):
    return np.array([(x, y, z) for x in range(-r, r + 1) for y in range(-r, r + 1) for z in range(-r, r + 1) if x * x + y * y + z * z <= r * r], np.int32).reshape(-1, 3)


def box(a, b, c, anchor=None):
    at = (a // 2, b // 2, c // 2) if anchor is None else anchor
    return np.array([(x - at[0], y - at[1], z - at[2]) for x in range(a) for y in range(b) for z in range(c)], np.int32).reshape(-1, 3)


def cross():
    return np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.int32)


def line(axis, lo, hi):
    e = np.zeros((hi - lo + 1, 3), np.int32)
    e[:, axis] = np.arange(lo, hi + 1)
    return e


def reflect(offsets):
    return -np.asarray(offsets, np.int32).reshape(-1, 3)


def random_element(rng, n, reach=REACH):
    """n offsets (duplicates possible) within `reach`"""
    return rng.integers(-reach, reach + 1, (n, 3)).astype(np.int32)


def source(S):
    """the three-band field of the cells tests: sparse, even and dense thirds side by side"""
    return three_band(S)
