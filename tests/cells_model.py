"""The numpy model of the cell calls (include/vrc.h: vrc_cells_step, vrc_cells_fill_random): the yardstick of
test_volume_cells_host.py, test_gpu_volume_cells.py and test_gpu_volume_cells_cpp.py.  Occupancy is dense [x, y, z] uint8.
The step pads with `outside`, sums the shifted slices and applies the masks; the hash is computed in uint32."""
import functools

import numpy as np

REPLACE, OR, ANDNOT = 0, 1, 2
FACES, ALL = 6, 26
STEPS = {n: [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (abs(dx) + abs(dy) + abs(dz) == 1 if n == FACES else (dx, dy, dz) != (0, 0, 0))] for n in (FACES, ALL)}
SMOOTH_BIRTH, SMOOTH_SURVIVE = sum(1 << c for c in range(14, 27)), sum(1 << c for c in range(13, 27))    # the majority of 27
SPECKS_SURVIVE = sum(1 << c for c in range(1, 7))


def finalise(u):
    """L(u) on a uint32 array, all arithmetic mod 2^32"""
    u = np.asarray(u, np.uint32).copy()
    u ^= u >> np.uint32(16)
    u *= np.uint32(0x7feb352d)
    u ^= u >> np.uint32(15)
    u *= np.uint32(0x846ca68b)
    u ^= u >> np.uint32(16)
    return u


def hash_field(seed, S):
    """h(x, y, z) = L(L(L(L(seed) ^ x) ^ y) ^ z) as uint32 [x, y, z]"""
    c = np.arange(S, dtype=np.uint32)
    hx = finalise(finalise(np.array([seed & 0xFFFFFFFF], np.uint32)) ^ c)
    hxy = finalise(hx[:, None] ^ c[None, :])
    return finalise(hxy[:, :, None] ^ c[None, None, :])


def threshold_of(density):
    return int(np.floor(density * 4294967296.0 + 0.5))


def random_set(seed, threshold, S):
    """R(p) = (h(p) < threshold), compared in 64 bits"""
    return (hash_field(seed, S).astype(np.uint64) < np.uint64(threshold)).astype(np.uint8) if threshold < (1 << 32) else np.ones((S, S, S), np.uint8)


def apply_op(dst, bits, op):
    return bits if op == REPLACE else (dst | bits) if op == OR else (dst & (1 - bits))


def fill_random(vol, seed, threshold, box=None, op=OR):
    """a copy of vol after vrc_cells_fill_random: box = lo x y z, hi x y z (exclusive), clipped; None = the whole volume"""
    S = vol.shape[0]
    out = vol.copy()
    lo, hi = ((0, 0, 0), (S, S, S)) if box is None else ([int(v) for v in box[:3]], [min(int(v), S) for v in box[3:]])
    if any(l >= h for l, h in zip(lo, hi)):
        return out
    view = out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    view[...] = apply_op(view, random_set(seed, threshold, S)[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], op)
    return out


def counts(vol, neighbours=ALL, outside=0):
    """c(p): the solid ones among the 6 or 26 neighbours of every voxel, those beyond the faces counting as `outside`"""
    S = vol.shape[0]
    padded = np.pad((np.asarray(vol) != 0).astype(np.uint8), 1, constant_values=int(outside))
    c = np.zeros((S, S, S), np.uint8)
    for dx, dy, dz in STEPS[neighbours]:
        c += padded[1 + dx:1 + dx + S, 1 + dy:1 + dy + S, 1 + dz:1 + dz + S]
    return c


def step(vol, birth, survive, neighbours=ALL, outside=0):
    """(the next state, the number of voxels that changed)"""
    c = counts(vol, neighbours, outside).astype(np.uint32)
    solid = np.asarray(vol) != 0
    out = np.where(solid, (np.uint32(survive) >> c) & 1, (np.uint32(birth) >> c) & 1).astype(np.uint8)
    return out, int((out != solid).sum())


def automaton(vol, steps, birth, survive, neighbours=ALL, outside=0):
    """(the state after at most `steps` steps, the steps that changed a voxel): ends at a step that changes nothing"""
    taken = 0
    while taken < steps:
        nxt, changed = step(vol, birth, survive, neighbours, outside)
        if not changed:
            break
        vol, taken = nxt, taken + 1
    return vol, taken


def smooth(vol, iterations=1, outside=0):
    return automaton(vol, iterations, SMOOTH_BIRTH, SMOOTH_SURVIVE, ALL, outside)[0]


def remove_specks(vol):
    return step(vol, 0, SPECKS_SURVIVE, FACES, 0)[0]


def caves(S, seed, density, steps):
    return smooth(random_set(seed, threshold_of(density), S), steps, 1)


@functools.lru_cache(maxsize=None)
def three_band(S):
    """fillRandom's hash with seed 7 at densities 0.12 / 0.5 / 0.88 on the thirds of x (third = 3 x // S): sparse, even and
    dense neighbourhoods side by side, so that every count occurs (test_volume_cells_host.py).  Shared: do not write to it."""
    band = (3 * np.arange(S)) // S
    h = hash_field(7, S).astype(np.uint64)
    t = np.array([threshold_of(d) for d in (0.12, 0.5, 0.88)], np.uint64)[band]
    vol = (h < t[:, None, None]).astype(np.uint8)
    vol.setflags(write=False)
    return vol
