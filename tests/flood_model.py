"""The yardstick of the flood tests: flood fill by connectivity as iterated masked dilation on a dense boolean array,
R <- R | (dilate(R) & M) until nothing changes.  Only the voxels added by the last step can add new ones, so each step
dilates that frontier alone, inside its bounding box -- the same sets step for step, at a cost that lets the model run on
512^3.  tests/test_volume_flood_host.py holds it against a plain breadth-first search."""
import numpy as np


def medium_set(medium, through_empty):
    """M: the solid voxels of the medium, or its empty ones (inside the volume: its faces are walls)"""
    medium = np.asarray(medium) != 0
    return ~medium if through_empty else medium


def dilate(F, connectivity):
    """F and its neighbours, no wrap-around: 6 = the OR of the six one-voxel shifts, 26 = three per-axis dilations"""
    if connectivity == 6:
        D = F.copy()
        D[1:] |= F[:-1]
        D[:-1] |= F[1:]
        D[:, 1:] |= F[:, :-1]
        D[:, :-1] |= F[:, 1:]
        D[:, :, 1:] |= F[:, :, :-1]
        D[:, :, :-1] |= F[:, :, 1:]
        return D
    assert connectivity == 26
    D = F
    for axis in range(3):
        E = D.copy()
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(1, None), slice(None, -1)
        E[tuple(a)] |= D[tuple(b)]
        E[tuple(b)] |= D[tuple(a)]
        D = E
    return D


def _bbox(A):
    lo, hi = [], []
    for axis in range(3):
        along = np.flatnonzero(A.any(axis=tuple(k for k in range(3) if k != axis)))
        if len(along) == 0:
            return None
        lo.append(int(along[0]))
        hi.append(int(along[-1]) + 1)
    return np.array(lo), np.array(hi)


def flood(medium, seeds, connectivity=6, through_empty=False):
    """uint8 [x, y, z]: the voxels of M joined to a seed in M by a chain of neighbours lying in M"""
    M = medium_set(medium, through_empty)
    S = np.array(M.shape)
    R = (np.asarray(seeds) != 0) & M
    box = _bbox(R)
    if box is None:
        return R.astype(np.uint8)
    lo, hi = box
    F = R[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].copy()
    while True:
        plo, phi = np.maximum(lo - 1, 0), np.minimum(hi + 1, S)
        P = np.zeros(phi - plo, bool)
        o = lo - plo
        P[o[0]:o[0] + F.shape[0], o[1]:o[1] + F.shape[1], o[2]:o[2] + F.shape[2]] = F
        sl = tuple(slice(int(a), int(b)) for a, b in zip(plo, phi))
        N = dilate(P, connectivity) & M[sl] & ~R[sl]
        box = _bbox(N)
        if box is None:
            return R.astype(np.uint8)
        R[sl] |= N
        nlo, nhi = box
        F = N[nlo[0]:nhi[0], nlo[1]:nhi[1], nlo[2]:nhi[2]]
        lo, hi = plo + nlo, plo + nhi


def flood_plain(medium, seeds, connectivity=6, through_empty=False):
    """the definition without the frontier: whole-array masked dilation to the fixed point (small volumes)"""
    M = medium_set(medium, through_empty)
    R = (np.asarray(seeds) != 0) & M
    while True:
        N = R | (dilate(R, connectivity) & M)
        if np.array_equal(N, R):
            return R.astype(np.uint8)
        R = N


def serpentine(S, pitch):
    """A one-voxel-wide path [x, y, z] that snakes through the whole S^3 volume: lines along z at every `pitch`-th y, joined
    alternately at their ends, layer after layer at every `pitch`-th x, the layers joined alternately too.  Returns the
    occupancy and the path's first voxel.  pitch >= 2 keeps the turns from touching, also by an edge or a corner."""
    assert pitch >= 2
    vol = np.zeros((S, S, S), np.uint8)
    ys = list(range(0, S, pitch))
    xs = list(range(0, S, pitch))
    y_up = z_up = True                   # the direction the path travels in along y (per layer) and along z (per line)
    for i, x in enumerate(xs):
        order = ys if y_up else ys[::-1]
        for j, y in enumerate(order):
            vol[x, y, :] = 1
            if j + 1 < len(order):
                y0, y1 = sorted((y, order[j + 1]))
                vol[x, y0:y1 + 1, S - 1 if z_up else 0] = 1
                z_up = not z_up
        if i + 1 < len(xs):
            vol[x:xs[i + 1] + 1, order[-1], S - 1 if z_up else 0] = 1
            z_up = not z_up
        y_up = not y_up
    return vol, (0, 0, 0)
