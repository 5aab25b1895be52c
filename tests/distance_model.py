"""The yardstick of the distance-field tests (include/vrc.h: vrc_volume_distance_field), numpy only.

The squared Euclidean distance transform is separable: the 1-D squared distance along z, then out[i] = min_j in[j] + (i-j)^2
along y and along x.  Each min-plus pass here is S vectorised steps (one per j) in int64 with a sentinel far above every
finite value, so nothing can overflow; the wall term of `outside` is applied at the end, as the header states it
(open_border).
tests/test_volume_distance_host.py holds this against the definition taken literally."""
import numpy as np

NONE = 0xFFFFFFFF
_INF = np.int64(1) << 40


def _minplus(G, axis):
    """out[i] = min_j G[j] + (i - j)^2 along `axis`; _INF stays _INF"""
    S = G.shape[axis]
    i = np.arange(S, dtype=np.int64)
    shape = [1, 1, 1]
    shape[axis] = S
    out = np.full(G.shape, _INF, np.int64)
    for j in range(S):
        out = np.minimum(out, np.take(G, [j], axis=axis) + ((i - j) ** 2).reshape(shape))
    return np.minimum(out, _INF)


def feature_set(vol, to_empty):
    return (np.asarray(vol) == 0) if to_empty else (np.asarray(vol) != 0)


def wall_term(S):
    """int64 [x, y, z]: min over the three axes a of (p_a + 1)^2 and (S - p_a)^2"""
    c = np.arange(S, dtype=np.int64)
    w = np.minimum(c + 1, S - c) ** 2
    return np.minimum(np.minimum(w[:, None, None], w[None, :, None]), w[None, None, :])


def field(vol, to_empty=False, outside=False):
    """uint32 [x, y, z]: the squared distance to the nearest voxel of F, NONE where F is empty"""
    F = feature_set(vol, to_empty)
    S = F.shape[0]
    assert F.shape == (S, S, S)
    G = np.where(F, np.int64(0), _INF)
    for axis in (2, 1, 0):
        G = _minplus(G, axis)
    D = np.where(G >= _INF, NONE, G).astype(np.uint32)
    return open_border(D) if outside else D


def open_border(D_inside):
    """the field with outside != 0 from the one with outside == 0: the minimum with the wall term (NONE is the largest uint32)"""
    return np.minimum(D_inside, wall_term(D_inside.shape[0]).astype(np.uint32))


def stats(D):
    """(max_d2, argmax as (x, y, z)): the largest finite value and the voxel of smallest dense index that holds it;
    (0, (0, 0, 0)) when no value is finite"""
    finite = D != NONE
    if not finite.any():
        return 0, (0, 0, 0)
    m = int(D[finite].max())
    first = int(np.flatnonzero((D == m).reshape(-1))[0])
    S = D.shape[0]
    return m, (first // (S * S), (first // S) % S, first % S)


def select(D, lo, hi):
    """uint8 [x, y, z]: lo <= D <= hi, NONE compared as the plain value"""
    return ((D >= lo) & (D <= hi)).astype(np.uint8)


def dilate(vol, r):
    return (np.asarray(vol) != 0) | (select(field(vol), 0, r * r) != 0)


def erode(vol, r, open_border=False):
    return (np.asarray(vol) != 0) & (select(field(vol, True, open_border), 0, r * r) == 0)


def hollow(vol, t):
    return (np.asarray(vol) != 0) & (select(field(vol, True), t * t + 1, NONE) == 0)
