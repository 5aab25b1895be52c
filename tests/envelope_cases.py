"""The cases of tests/test_gpu_volume_envelope.py: volumes at 128^3, 256^3 and 512^3 on which the lower-envelope stacks of
k_distance_minplus (vrc_distance.hip) and k_fracture_minplus (vrc_fracture.hip) grow deep AND pop, in LDS and in device
memory, and on which the line loop of both kernels takes its second step.  Beside the scenes: references that are no
lower-envelope walk (scipy's feature transform with the squared distance recomputed in int64, a closed form for unions of
product sets, a packed min-plus for the cells, a closed form for product grids of sites), the launch geometry of the kernels
restated in Python from the code as it stands, each with the line it was read off, and a plain restatement of the first
walk, so that the host test (tests/test_volume_envelope_cases_host.py) can hold the cases to the regime they are meant for.
numpy, scipy.ndimage and Python integers only."""
import functools

import numpy as np

NONE = 0xFFFFFFFF                    # VRC_DISTANCE_NONE, VRC_NO_COMPONENT
SIZES = (128, 256)
SCENES = ("slant", "ball", "products")


# ---- the launch geometry --------------------------------------------------------------------------------------------

GROUP = 256                          # vrc_distance.hip:38, vrc_fracture.hip:54: lanes of the z passes
LANES = 64                           # vrc_distance.hip:39, vrc_fracture.hip:55: lines per workgroup of the min-plus passes
LDS_STACK_MAX_DEPTH = 7              # vrc_distance.hip:40, vrc_fracture.hip:56
WAVES_PER_CU = 8                     # vrc_distance.hip:41, vrc_fracture.hip:57
Z_GROUPS_PER_CU = 16                 # vrc_distance.hip:276, vrc_fracture.hip:255: z_cap = cu_count * 16
CU_COUNT = 256                       # an MI355X


def z_columns_per_step(S):
    """vrc_distance.hip:45"""
    return 2048 // S if S >= GROUP else GROUP // S


def distance_z_groups(depth, cu_count=CU_COUNT):
    """vrc_distance.hip:274-277: (workgroups wanted, workgroups launched) of k_distance_z"""
    S = 1 << depth
    cpi = z_columns_per_step(S)
    want = (S * S + cpi - 1) // cpi
    return want, min(want, max(cu_count, 1) * Z_GROUPS_PER_CU)


def words_per_column(S):
    """vrc_distance.hip:52"""
    return S >> 5 if S >= 32 else 1


def minplus_groups(depth, cu_count=CU_COUNT):
    """vrc_distance.hip:250-255, vrc_fracture.hip:227-232"""
    want = ((1 << (2 * depth)) + LANES - 1) // LANES
    return min(want, max(cu_count, 1) * WAVES_PER_CU)


def line_steps(depth, cu_count=CU_COUNT):
    """vrc_distance.hip:132, vrc_fracture.hip:157: the steps of for (l0 = blockIdx.x * LANES; l0 < lines; l0 += gridDim.x * LANES)
    that the first workgroup takes"""
    want = ((1 << (2 * depth)) + LANES - 1) // LANES
    return -(-want // minplus_groups(depth, cu_count))


def stacks_in_lds(depth):
    """vrc_distance.hip:280, vrc_fracture.hip:259"""
    return depth <= LDS_STACK_MAX_DEPTH


def fracture_z_geometry(depth, cu_count=CU_COUNT):
    """vrc_fracture.hip:76 and 253-256: (W, chunks, units, workgroups launched) of k_fracture_z"""
    S = 1 << depth
    W = 64 if S < 64 else S
    units = (1 << (3 * depth)) // W
    groups = (units + GROUP // 64 - 1) // (GROUP // 64)
    return W, W >> 6, units, min(groups, max(cu_count, 1) * Z_GROUPS_PER_CU)


# ---- the first walk, restated ---------------------------------------------------------------------------------------

def first_walk(f, strict, reload_offset=2):
    """vrc_distance.hip:139-162 (strict=False: a parabola is popped on >=) and vrc_fracture.hip:165-190 (strict=True: on >
    alone) over one line of partial squared distances f (NONE: no entry): (the stack as a list of positions, the greatest
    top, the longest pop cascade of one push, the pops).  Python integers.  reload_offset is for experiments with a wrong
    walk: the entry read back after a pop, top - 2 in the kernels."""
    stack, F = [], []
    va = Fa = vb = Fb = 0
    greatest = cascade = pops = 0
    for q, fq in enumerate(f):
        fq = int(fq)
        if fq == NONE:
            continue
        Fq = fq + q * q
        run = 0
        while len(stack) >= 2:
            lhs, rhs = (Fb - Fa) * (q - vb), (Fq - Fb) * (vb - va)
            if not (lhs > rhs if strict else lhs >= rhs):
                break
            stack.pop()
            F.pop()
            run += 1
            vb, Fb = va, Fa
            if len(stack) >= 2:
                k = len(stack) - reload_offset
                va, Fa = stack[k], F[k]
        stack.append(q)
        F.append(Fq)
        va, Fa, vb, Fb = vb, Fb, q, Fq
        greatest = max(greatest, len(stack))
        cascade = max(cascade, run)
        pops += run
    return stack, greatest, cascade, pops


def second_walk(f, stack):
    """vrc_distance.hip:164-187: the envelope's value at every i off the stack of first_walk; NONE for an empty stack"""
    S = len(f)
    if not stack:
        return [NONE] * S
    out, k = [], 0
    for i in range(S):
        val = int(f[stack[k]]) + (i - stack[k]) ** 2
        while k + 1 < len(stack):
            nxt = int(f[stack[k + 1]]) + (i - stack[k + 1]) ** 2
            if nxt > val:
                break
            k, val = k + 1, nxt
        out.append(val)
    return out


def walk_stats(lines, strict):
    """(n, 3) per line of an (n, S) array: the greatest top, the longest cascade, the pops"""
    return np.array([first_walk(f.tolist(), strict)[1:] for f in lines], np.int64).reshape(-1, 3)


# ---- the scenes -----------------------------------------------------------------------------------------------------

SPECK_DENSITY = 5e-4
SEED = 7                             # of the specks
PRODUCT_SEED = 61                    # of the products: chosen so that the scenes alone meet the host test's conditions


def axis_sets(S, seed=PRODUCT_SEED, K=6):
    """the union-of-products scene as K triples (A, B, C) of bool (S,) arrays: densities drawn from 0.02, 0.1 and 0.5, every
    set non-empty"""
    rng = np.random.default_rng([seed, S])
    out = []
    for _ in range(K):
        triple = []
        for _ in range(3):
            a = rng.random(S) < rng.choice([0.02, 0.1, 0.5])
            if not a.any():
                a[rng.integers(0, S)] = True
            triple.append(a)
        out.append(tuple(triple))
    return out


def products_volume(sets):
    S = len(sets[0][0])
    vol = np.zeros((S, S, S), bool)
    for A, B, C in sets:
        vol |= A[:, None, None] & B[None, :, None] & C[None, None, :]
    return vol.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(name, S, seed=SEED):
    """uint8 [x, y, z], the solid voxels.  slant: z == y and random specks; ball: the complement of a ball of radius 0.44 S
    about (S/2, S/2, S/2), |p - c|^2 >= (0.44 S)^2 held in integers; products: axis_sets.  Shared: do not write to it."""
    if name == "slant":
        rng = np.random.default_rng([seed, S, 1])
        vol = (rng.random((S, S, S)) < SPECK_DENSITY).astype(np.uint8)
        c = np.arange(S)
        vol[:, c, c] = 1
    elif name == "ball":
        c = (np.arange(S, dtype=np.int64) - S // 2) ** 2
        d2 = c[:, None, None] + c[None, :, None] + c[None, None, :]
        vol = (10000 * d2 >= (44 * S) ** 2).astype(np.uint8)
    else:
        assert name == "products"
        vol = products_volume(axis_sets(S))
    vol.setflags(write=False)
    return vol


def features_of(vol, to_empty):
    return (vol == 0) if to_empty else (vol != 0)


# ---- references for the distance field ------------------------------------------------------------------------------

def edt_reference(F):
    """uint32 [x, y, z]: the squared distance to the nearest voxel of the bool set F, from the feature transform of
    scipy.ndimage (the nearest feature's INDEX per voxel) with the squared distance recomputed in int64; NONE where F is
    empty"""
    from scipy import ndimage
    S = F.shape[0]
    if not F.any():
        return np.full(F.shape, NONE, np.uint32)
    index = ndimage.distance_transform_edt(~F, return_distances=False, return_indices=True)
    assert F[tuple(index)].all()                                             # every index names a feature voxel
    d2 = np.zeros(F.shape, np.int64)
    for axis in range(3):
        shape = [1, 1, 1]
        shape[axis] = S
        d = index[axis].astype(np.int64) - np.arange(S, dtype=np.int64).reshape(shape)
        d2 += d * d
    return d2.astype(np.uint32)


@functools.lru_cache(maxsize=2)
def scene_field(name, S, to_empty):
    """edt_reference of a scene's feature set, outside == 0.  Shared: do not write to it."""
    D = edt_reference(features_of(scene(name, S), to_empty))
    D.setflags(write=False)
    return D


def distance_1d(A):
    """int64 (S,): the distance of every coordinate to the nearest member of the non-empty bool (S,) set A, by brute force"""
    c = np.arange(len(A), dtype=np.int64)
    return np.abs(c[:, None] - c[A][None, :]).min(axis=1)


def products_field(sets):
    """uint32 [x, y, z]: min over k of dA_k(x)^2 + dB_k(y)^2 + dC_k(z)^2, the distance field of the union of the products"""
    S = len(sets[0][0])
    D = np.full((S, S, S), NONE, np.uint32)
    tmp = np.empty((S, S, S), np.uint32)
    for A, B, C in sets:
        a, b, c = [(distance_1d(X) ** 2).astype(np.uint32) for X in (A, B, C)]
        np.add(a[:, None, None], b[None, :, None], out=tmp)
        np.add(tmp, c[None, None, :], out=tmp)
        np.minimum(D, tmp, out=D)
    return D


def open_border_in_place(D):
    """distance_model.open_border without a second array: the minimum with the wall term"""
    S = D.shape[0]
    c = np.arange(S, dtype=np.int64)
    w = (np.minimum(c + 1, S - c) ** 2).astype(np.uint32)
    np.minimum(D, w[:, None, None], out=D)
    np.minimum(D, w[None, :, None], out=D)
    np.minimum(D, w[None, None, :], out=D)
    return D


def stats_of_finite(D):
    """distance_model.stats for a field without NONE, without copying it"""
    m = int(D.max())
    first = int(np.argmax(D.reshape(-1) == m))
    S = D.shape[0]
    return m, (first // (S * S), (first // S) % S, first % S)


def product_count(sets):
    """the voxels of the union of the products, by inclusion of one x layer at a time"""
    total = 0
    for x in range(len(sets[0][0])):
        layer = np.zeros((len(sets[0][1]), len(sets[0][2])), bool)
        for A, B, C in sets:
            if A[x]:
                layer |= B[:, None] & C[None, :]
        total += int(layer.sum())
    return total


def runs_of(A):
    """[(start, end)] of the runs of the bool (S,) array A"""
    edge = np.flatnonzero(np.diff(np.concatenate([[0], A.astype(np.int8), [0]])))
    return list(zip(edge[0::2].tolist(), edge[1::2].tolist()))


def product_boxes(A, B, C):
    """the product A x B x C as two lists of boxes [x0, y0, z0, x1, y1, z1]: the slabs of A to set, then the slabs of the
    complements of B and C to clear"""
    S = len(A)
    fill = [[a, 0, 0, b, S, S] for a, b in runs_of(A)]
    clear = [[0, a, 0, S, b, S] for a, b in runs_of(~B)] + [[0, 0, a, S, S, b] for a, b in runs_of(~C)]
    return np.array(fill, np.uint32).reshape(-1, 6), np.array(clear, np.uint32).reshape(-1, 6)


# ---- the partial fields the walks read ------------------------------------------------------------------------------

_FAR = np.int64(1) << 40


def z_pass(F):
    """int64 [x, y, z]: the squared distance to the nearest voxel of F in the same z column, _FAR where the column has none;
    two running extrema, no envelope"""
    S = F.shape[0]
    z = np.arange(S, dtype=np.int64)
    below = np.maximum.accumulate(np.where(F, z, -_FAR), axis=2)
    above = np.minimum.accumulate(np.where(F, z, _FAR)[:, :, ::-1], axis=2)[:, :, ::-1]
    d = np.minimum(z - below, above - z)
    return np.where(d >= _FAR // 2, _FAR, d * d)


def as_entries(lines):
    """int64 lines with _FAR as (n, S) arrays the walks read: NONE for no entry"""
    return np.where(lines >= _FAR, NONE, lines)


def y_lines(g0, picks):
    """the lines the y pass reads, l = x * S + z (vrc_distance.hip:135): (n, S) over j"""
    S = g0.shape[0]
    return as_entries(np.stack([g0[l // S, :, l % S] for l in picks]))


def x_lines(g0, picks):
    """the lines the x pass reads, l = y * S + z: g1(j, y, z) = min_j' g0(j, j', z) + (y - j')^2 by brute force"""
    S = g0.shape[0]
    c = np.arange(S, dtype=np.int64)
    out = []
    for l in picks:
        y, z = l // S, l % S
        out.append(np.minimum((g0[:, :, z] + (y - c)[None, :] ** 2).min(axis=1), _FAR))
    return as_entries(np.stack(out))


def sampled_lines(S, count, seed=1):
    """`count` line numbers, the first and the last line among them"""
    rng = np.random.default_rng([seed, S])
    picks = rng.choice(S * S, count, replace=False)
    picks[0], picks[1] = 0, S * S - 1
    return np.unique(picks)


# ---- sites and the references for the cells -------------------------------------------------------------------------

MAX_SITES = 1 << 17


def scene_sites(name, S, seed=SEED):
    """(n, 3) int32: the scene's solid voxels in dense-index order; beyond MAX_SITES the
    voxels of whole x layers, evenly spaced, so that the lines of the y pass inside a kept layer are the scene's own"""
    vol = scene(name, S, seed)
    sites = np.argwhere(vol)
    if len(sites) > MAX_SITES:
        per_layer = vol.reshape(S, -1).sum(axis=1, dtype=np.int64)
        step = 1
        while per_layer[::step].sum() > MAX_SITES:
            step += 1
        sites = sites[sites[:, 0] % step == 0]
    return np.ascontiguousarray(sites, np.int32)


def shuffled(sites, seed=3):
    return np.ascontiguousarray(sites[np.random.default_rng(seed).permutation(len(sites))])


def site_set(sites, S):
    F = np.zeros((S, S, S), bool)
    F[tuple(np.asarray(sites, np.int64).T)] = True
    return F


_BIG = np.int64(1) << 62


def packed_start(S, sites):
    """int64 [x, y, z]: (0 << 32) | the lowest index of a site at the voxel, _BIG where there is none; sites outside are skipped"""
    s = np.asarray(sites, np.int64).reshape(-1, 3)
    inside = ((s >= 0) & (s < S)).all(axis=1)
    P = np.full(S ** 3, _BIG, np.int64)
    np.minimum.at(P, ((s[inside, 0] * S + s[inside, 1]) * S + s[inside, 2]), np.flatnonzero(inside).astype(np.int64))
    return P.reshape(S, S, S)


def packed_minplus(P, axis, window=None):
    """out[i] = min_j P[j] + ((i - j)^2 << 32) along `axis`, the minimum of (d2, index) pairs as one int64; with a window only
    |i - j| <= window takes part"""
    S = P.shape[axis]
    out = P.copy()
    if window is None:
        i = np.arange(S, dtype=np.int64)
        shape = [1, 1, 1]
        shape[axis] = S
        tmp = np.empty_like(P)
        for j in range(S):
            np.add(np.take(P, [j], axis=axis), (((i - j) ** 2) << 32).reshape(shape), out=tmp)
            np.minimum(out, tmp, out=out)
        return out
    for d in range(1, min(window, S - 1) + 1):
        near, far = [slice(None)] * 3, [slice(None)] * 3
        near[axis], far[axis] = slice(0, S - d), slice(d, S)
        near, far = tuple(near), tuple(far)
        cost = np.int64(d * d) << 32
        lower, upper = P[far] + cost, P[near] + cost
        np.minimum(out[near], lower, out=out[near])
        np.minimum(out[far], upper, out=out[far])
    return out


def packed_field(S, sites, window=None):
    """int64 [x, y, z]: (the least squared distance to a site << 32) | the lowest index among the sites at that distance"""
    P = packed_start(S, sites)
    for axis in (2, 1, 0):
        P = packed_minplus(P, axis, window)
    return P


def packed_cells(S, sites, max_d2=NONE, window=None):
    """uint32 [x, y, z]: fracture_model.cells by three packed min-plus passes -- the lowest index among the nearest sites
    comes with the minimum.  With a window, max_d2 must not exceed window^2: every site within the cut-off lies within the
    window on every axis, so the result is exact wherever a cell is reported and NONE elsewhere"""
    assert window is None or max_d2 <= window * window
    return cells_of_packed(packed_field(S, sites, window), max_d2)


def cells_of_packed(P, max_d2=NONE):
    cell = (P & 0xFFFFFFFF).astype(np.uint32)
    cell[P >= _BIG] = NONE
    if max_d2 != NONE:
        cell[(P >> 32) > max_d2] = NONE
    return cell


def tied_voxels(S, sites, window):
    """the voxels within `window` of a site with several nearest sites at different coordinates: where the packed minimum
    under the reversed index order names a site somewhere else"""
    s = np.asarray(sites, np.int64).reshape(-1, 3)
    first = packed_cells(S, s, window * window, window)
    last = packed_cells(S, s[::-1], window * window, window)
    seen = first != NONE
    assert np.array_equal(seen, last != NONE)
    a, b = s[first[seen].astype(np.int64)], s[::-1][last[seen].astype(np.int64)]
    return int((a != b).any(axis=-1).sum())


class Grid:
    """axes (three sorted coordinate arrays), table (the site index of every grid point), extras ((3 T, 3) coordinates of the
    sites off the grid, three to a triple: outer, middle, outer), extra_index ((3 T,) their indices), centres ((T, 3) the
    voxel at which a triple's three parabolas meet), sites ((n, 3) int32 in index order)"""


GRID_COUNTS = {256: (40, 64, 8), 512: (160, 200, 10)}
TRIPLES = 40
TRIPLE_REACH = 3                     # the greatest h of a triple
TRIPLE_CLEAR = 8                     # a triple's z layers keep this distance from the grid's


def grid_sites(S, counts, seed=5, triples=TRIPLES):
    """a product grid X x Y x Z of sites, counts = (|X|, |Y|, |Z|) random coordinates per axis, and `triples` collinear triples
    off the grid, all under shuffled indices.  Along a line of the grid f is constant, the parabolas c + (i - j)^2 never meet
    three at a point and popping on >= cannot be told from popping on >; a triple is what tells them apart
    (tests/test_gpu_volume_fracture.py: tie_cases): two sites 2h apart along x (the even triples) or y (the odd ones) and a
    third in the middle, h aside -- along y, or along z -- in a z layer far enough from the grid's that the three are the
    nearest sites of the voxel between the outer two.  All three are h^2 from that voxel and the middle one's parabola is
    lowest nowhere else, so with the lowest index in the middle the voxel is the middle site's only by the tie"""
    rng = np.random.default_rng([seed, S])
    g = Grid()
    g.axes = [np.sort(rng.choice(S, n, replace=False)).astype(np.int64) for n in counts]
    n_grid = int(np.prod(counts))
    c = np.arange(S, dtype=np.int64)
    dz = np.abs(c[:, None] - g.axes[2][None, :]).min(axis=1)
    free = np.flatnonzero((dz >= TRIPLE_CLEAR) & (c >= 8) & (c < S - 8))
    extras, centres = [], []
    for t in range(triples):
        h = int(rng.integers(1, TRIPLE_REACH + 1))
        u, v, z0 = int(rng.integers(8, S - 8)), int(rng.integers(8, S - 8)), int(rng.choice(free))
        if t % 2 == 0:                   # along x, the middle h aside in y: they meet on the x line through (., v, z0)
            extras += [(u - h, v, z0), (u, v + h, z0), (u + h, v, z0)]
        else:                            # along y, the middle h aside in z: they meet on the y line through (u, ., z0)
            extras += [(u, v - h, z0), (u, v, z0 + h), (u, v + h, z0)]
        centres.append((u, v, z0))
    g.extras, g.centres = np.array(extras, np.int64).reshape(-1, 3), np.array(centres, np.int64).reshape(-1, 3)
    perm = rng.permutation(n_grid + len(g.extras)).astype(np.uint32)
    g.table, g.extra_index = perm[:n_grid].reshape(counts), perm[n_grid:]
    points = np.stack(np.meshgrid(*g.axes, indexing="ij"), axis=-1).reshape(-1, 3)
    g.sites = np.empty((len(perm), 3), np.int32)
    g.sites[g.table.reshape(-1)] = points
    g.sites[g.extra_index] = g.extras
    return g


def tie_won_triples(g, S):
    """the triples whose centre the closed form gives to the middle site while the middle site has the lowest index of the three:
    a walk that pops on >= gives these voxels to an outer site"""
    cell = grid_cells_at(g, S, g.centres)
    idx = g.extra_index.reshape(-1, 3).astype(np.int64)
    return np.flatnonzero((cell == idx[:, 1]) & (idx[:, 1] < idx[:, 0]) & (idx[:, 1] < idx[:, 2]))


def nearest_two(axis_coords, S):
    """(S, 2) positions in the sorted coordinate list of the nearest coordinate to every p: twice the same one, or the two
    that are equally near"""
    c = np.arange(S, dtype=np.int64)
    d = np.abs(c[:, None] - axis_coords[None, :])
    least = d.min(axis=1)
    first = np.argmax(d == least[:, None], axis=1)
    last = len(axis_coords) - 1 - np.argmax((d == least[:, None])[:, ::-1], axis=1)
    return np.stack([first, last], axis=1)


def grid_cells_at(g, S, xyz):
    """uint32 (n,): the cell of every voxel of the (n, 3) list by the closed form: the nearest coordinate per axis, and of the up
    to 8 combinations of equally near ones the lowest index"""
    xyz = np.asarray(xyz, np.int64)
    near = [nearest_two(a, S) for a in g.axes]
    out = np.full(len(xyz), NONE, np.uint32)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                np.minimum(out, g.table[near[0][xyz[:, 0], a], near[1][xyz[:, 1], b], near[2][xyz[:, 2], c]], out=out)
    # the sites off the grid, by brute force: the minimum of (d2, index) packed as one int64
    d2 = sum((xyz[:, k] - g.axes[k][near[k][xyz[:, k], 0]]) ** 2 for k in range(3))
    best = (d2 << 32) | out.astype(np.int64)
    reach = int(np.sqrt(float(d2.max()))) + 1                                # no site farther off than this wins a voxel of the list
    order = np.argsort(xyz[:, 0], kind="stable")
    xs = xyz[order, 0]
    for p, i in zip(g.extras, g.extra_index.astype(np.int64)):
        some = order[np.searchsorted(xs, p[0] - reach):np.searchsorted(xs, p[0] + reach, side="right")]
        best[some] = np.minimum(best[some], (((xyz[some] - p) ** 2).sum(axis=1) << 32) | i)
    return (best & 0xFFFFFFFF).astype(np.uint32)


def grid_cells(g, S):
    """grid_cells_at of every voxel, [x, y, z]; a site off the grid is tried within the grid's greatest distance of it"""
    near = [nearest_two(a, S) for a in g.axes]
    out = np.full((S, S, S), NONE, np.uint32)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                np.minimum(out, g.table[np.ix_(near[0][:, a], near[1][:, b], near[2][:, c])], out=out)
    c = np.arange(S, dtype=np.int64)
    d1 = [(c - g.axes[k][near[k][:, 0]]) ** 2 for k in range(3)]
    best = ((d1[0][:, None, None] + d1[1][None, :, None] + d1[2][None, None, :]) << 32) | out.astype(np.int64)
    reach = int(np.sqrt(float(sum(int(d.max()) for d in d1)))) + 1
    for p, i in zip(g.extras.tolist(), g.extra_index.tolist()):
        box = tuple(slice(max(0, v - reach), min(S, v + reach + 1)) for v in p)
        d = [(c[s] - v) ** 2 for s, v in zip(box, p)]
        packed = ((d[0][:, None, None] + d[1][None, :, None] + d[2][None, None, :]) << 32) | i
        np.minimum(best[box], packed, out=best[box])
    return (best & 0xFFFFFFFF).astype(np.uint32)


def probes_512(seed=9, S=512, stride=8, random=1 << 21):
    """(n, 3) uint32: a lattice of the given stride and random voxels -- the second step of the line loop writes x >= 256 in the
    y pass and y >= 256 in the x pass"""
    rng = np.random.default_rng(seed)
    c = np.arange(0, S, stride)
    lattice = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.concatenate([lattice, rng.integers(0, S, (random - len(lattice), 3))]).astype(np.uint32)


# ---- the pieces of the clearance case -------------------------------------------------------------------------------

def clearance_case(S=256, count=20, seed=21):
    """`count` boxes of a 32^3 volume, apart from each other, as (debris, offsets (count, 3): where each piece's voxels go)"""
    rng = np.random.default_rng(seed)
    debris = np.zeros((32, 32, 32), np.uint8)
    k = 0
    for x in range(0, 32, 8):
        for y in range(0, 32, 8):
            for z in range(0, 32, 16):
                if k < count:
                    size = rng.integers(2, 7, 3)
                    debris[x:x + size[0], y:y + size[1], z:z + size[2]] = 1
                    k += 1
    offsets = rng.integers(0, S - 32, (count, 3)).astype(np.int64)
    offsets[0], offsets[1] = (0, 0, 0), (S - 32, S - 32, S - 32)
    return debris, offsets
