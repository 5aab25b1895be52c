"""The yardstick of the connected-component tests (include/vrc.h: vrc_volume_label_components), numpy only.

Every voxel of M starts with its own key, 8 B + (z&1) 4 + (y&1) 2 + (x&1) with B = ((x/2) n + y/2) n + z/2 its brick
index.  A label is always the key of a voxel of the same piece whose own label is no larger.  A step takes, for every voxel,
the smallest label among itself and its neighbours in M (the flood model's shifts with a minimum in place of the OR), hands
it on to the voxel its old label names, and then follows labels as pointers until that changes nothing.  At the fixed point
all neighbours agree, so a piece carries one label, a key of the piece that is no larger than the key of any of its
voxels: the smallest key of the piece, its representative.  Pieces are numbered by ascending representative key.
tests/test_volume_components_host.py holds this against a plain breadth-first search."""
import numpy as np

import flood_model

NO_COMPONENT = 0xFFFFFFFF
RECORD = np.dtype([("first", "<u4", 3), ("lo", "<u4", 3), ("hi", "<u4", 3), ("reserved", "<u4"), ("voxels", "<u8")])


def keys(S):
    """int64 [x, y, z]: every voxel's key"""
    n = S // 2
    c = np.arange(S, dtype=np.int64)
    x, y, z = c[:, None, None], c[None, :, None], c[None, None, :]
    return 8 * (((x >> 1) * n + (y >> 1)) * n + (z >> 1)) + (z & 1) * 4 + (y & 1) * 2 + (x & 1)


def _min_with_neighbours(L, connectivity):
    """L and its neighbours' minimum, no wrap-around: flood_model.dilate with np.minimum"""
    def along(D, axis):
        E = D.copy()
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(1, None), slice(None, -1)
        E[tuple(a)] = np.minimum(E[tuple(a)], D[tuple(b)])
        E[tuple(b)] = np.minimum(E[tuple(b)], D[tuple(a)])
        return E
    if connectivity == 6:
        return np.minimum(np.minimum(along(L, 0), along(L, 1)), along(L, 2))
    assert connectivity == 26
    return along(along(along(L, 0), 1), 2)


def label(medium, connectivity=6, through_empty=False):
    """(ids uint32 [x, y, z] with NO_COMPONENT outside M, records in id order)"""
    M = flood_model.medium_set(medium, through_empty)
    S = M.shape[0]
    assert M.shape == (S, S, S)
    K = keys(S)
    big = np.int64(S) ** 3
    where = np.empty(S ** 3 + 1, np.int64)          # key -> flat index of its voxel; `big` -> a slot that holds `big`
    where[K.reshape(-1)] = np.arange(S ** 3)
    where[big] = S ** 3
    L = np.append(np.where(M, K, big).reshape(-1), big)       # flat, [x, y, z] order, plus the slot of `big`
    while True:
        N = np.append(_min_with_neighbours(L[:-1].reshape(S, S, S), connectivity).reshape(-1), big)
        N[:-1][~M.reshape(-1)] = big
        # the voxel whose key is v's label takes the smallest label seen around v, then labels are followed as pointers
        np.minimum.at(N, where[L], N.copy())
        while True:
            J = N[where[N]]
            if np.array_equal(J, N):
                break
            N = J
        if np.array_equal(N, L):
            break
        L = N
    L = L[:-1].reshape(S, S, S)
    reps = np.unique(L[M])                          # ascending representative keys
    ids = np.full((S, S, S), NO_COMPONENT, np.uint32)
    ids[M] = np.searchsorted(reps, L[M]).astype(np.uint32)
    return ids, records_of(ids, K)


def records_of(ids, K=None):
    """the records of a labelling: first = the voxel of minimum key, the bounding box, the voxel count"""
    S = ids.shape[0]
    K = keys(S) if K is None else K
    inside = ids != NO_COMPONENT
    xyz = np.argwhere(inside)
    i = ids[inside].astype(np.int64)
    C = int(i.max()) + 1 if len(i) else 0
    rec = np.zeros(C, RECORD)
    rec["voxels"] = np.bincount(i, minlength=C)
    lo = np.full((C, 3), S, np.int64)
    hi = np.zeros((C, 3), np.int64)
    best = np.full(C, np.int64(S) ** 3)
    np.minimum.at(best, i, K[inside])
    for a in range(3):
        np.minimum.at(lo[:, a], i, xyz[:, a])
        np.maximum.at(hi[:, a], i, xyz[:, a] + 1)
    rec["lo"], rec["hi"] = lo, hi
    first = xyz[K[inside] == best[i]]               # one voxel per component, in some order
    rec["first"][ids[tuple(first.T)]] = first
    return rec


def select(ids, keep):
    """uint8 [x, y, z]: the voxels of the pieces with keep[id] != 0"""
    keep = np.append(np.asarray(keep) != 0, False)
    return keep[np.where(ids == NO_COMPONENT, len(keep) - 1, ids)].astype(np.uint8)


def despeckle(medium, min_voxels, connectivity=6):
    """the medium without its solid pieces of fewer than min_voxels voxels"""
    ids, rec = label(medium, connectivity)
    return select(ids, rec["voxels"] >= min_voxels)
