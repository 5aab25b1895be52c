"""The yardstick of the Voronoi-fracture tests (include/vrc.h: vrc_fracture_label), numpy only.

cells() is brute force over the sites: the squared distance of every voxel to every in-volume site in int64, the argmin of
(d2, index) -- a later site replaces an earlier one only where it is STRICTLY nearer -- and the cut-off.  label() is the
labelling of tests/components_model.py with one more condition: a voxel takes a neighbour's label only if the neighbour
carries its own cell value; every one of the 6 or 26 offsets is taken on its own, because a diagonal step asks nothing of the
voxels beside it.  tests/test_volume_fracture_host.py holds cells() against a literal per-voxel, per-site loop and label()
against a breadth-first search."""
import itertools

import numpy as np

import components_model
import flood_model

NONE = 0xFFFFFFFF          # VRC_NO_COMPONENT as a cell, VRC_DISTANCE_NONE as max_d2


def cells(S, sites, max_d2=NONE):
    """uint32 [x, y, z]: the index of the nearest in-volume site, the lowest among several nearest; NONE where there is
    none or the least squared distance exceeds max_d2 (NONE: no cut-off)"""
    sites = np.asarray(sites, np.int64).reshape(-1, 3)
    c = np.arange(S, dtype=np.int64)
    best = np.full((S, S, S), np.iinfo(np.int64).max, np.int64)
    cell = np.full((S, S, S), NONE, np.uint32)
    for i, (sx, sy, sz) in enumerate(sites):
        if not (0 <= sx < S and 0 <= sy < S and 0 <= sz < S):
            continue
        d2 = ((c - sx) ** 2)[:, None, None] + ((c - sy) ** 2)[None, :, None] + ((c - sz) ** 2)[None, None, :]
        nearer = d2 < best
        best[nearer] = d2[nearer]
        cell[nearer] = i
    if max_d2 != NONE:
        cell[best > max_d2] = NONE
    return cell


def offsets_of(connectivity):
    assert connectivity in (6, 26)
    every = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
    return [d for d in every if connectivity == 26 or sum(map(abs, d)) == 1]


def _min_with_neighbours(L, cell, connectivity, big):
    """L and the minimum over the neighbours of the same cell, no wrap-around"""
    S = L.shape[0]
    E = L.copy()
    for d in offsets_of(connectivity):
        a = tuple(slice(max(0, -k), S - max(0, k)) for k in d)          # the voxel
        b = tuple(slice(max(0, k), S - max(0, -k)) for k in d)          # its neighbour at +d
        E[a] = np.minimum(E[a], np.where(cell[a] == cell[b], L[b], big))
    return E


def label_cells(M, cell, connectivity):
    """(ids, records) of the pieces of the boolean M cut along the borders of `cell`"""
    S = M.shape[0]
    K = components_model.keys(S)
    big = np.int64(S) ** 3
    where = np.empty(S ** 3 + 1, np.int64)
    where[K.reshape(-1)] = np.arange(S ** 3)
    where[big] = S ** 3
    L = np.append(np.where(M, K, big).reshape(-1), big)
    while True:
        N = np.append(_min_with_neighbours(L[:-1].reshape(S, S, S), cell, connectivity, big).reshape(-1), big)
        N[:-1][~M.reshape(-1)] = big
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
    reps = np.unique(L[M])
    ids = np.full((S, S, S), components_model.NO_COMPONENT, np.uint32)
    ids[M] = np.searchsorted(reps, L[M]).astype(np.uint32)
    return ids, components_model.records_of(ids, K)


def label(medium, sites, connectivity=6, through_empty=False, max_d2=NONE):
    """(ids uint32 [x, y, z] with NONE outside M, records in id order, the cell of every piece as uint32)"""
    M = flood_model.medium_set(medium, through_empty)
    cell = cells(M.shape[0], sites, max_d2)
    ids, rec = label_cells(M, cell, connectivity)
    return ids, rec, piece_sites(rec, cell)


def piece_sites(rec, cell):
    """the cell at every record's representative"""
    first = rec["first"].astype(np.int64).reshape(-1, 3)
    return cell[first[:, 0], first[:, 1], first[:, 2]].astype(np.uint32)
