"""numpy / Python-integer restatement of the two rules of vrc_raster_mesh (include/vrc.h), the yardstick of the surface
voxelisation tests, written from the header's text and by brute force: TOUCHED holds the 13-axis predicate against every voxel
of the triangle's clipped bounding box, THIN the cover rule and the crossing against every column of the volume, per axis.
Fixed point with 64 units per voxel: voxel p is the closed cube [64p, 64p + 64]^3, its centre 64p + 32.  int64 throughout (every
quantity stays below 2^57); touches_int is the predicate for one voxel in Python integers.  tests/test_raster_host.py holds
the model to facts that do not come from the predicate."""
import numpy as np

UNIT = 64
HALF = 32
LIMIT = 1 << 17             # a triangle with a coordinate beyond +-LIMIT is dropped
TOUCHED, THIN = 0, 1


def vertices(t):
    """the three vertices of a triangle of 9 integers as lists of Python integers; None for a dropped triangle"""
    c = [int(q) for q in t]
    if any(abs(q) > LIMIT for q in c):
        return None
    return c[0:3], c[3:6], c[6:9]


def cross(u, w):
    return [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]


def normal(A, B, C):
    return cross([B[i] - A[i] for i in range(3)], [C[i] - A[i] for i in range(3)])


def axes_of(A, B, C):
    """the 13 axes: the unit axes, n, and e_a x (Q - P) for the three edges and the three unit axes"""
    units = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    L = list(units) + [normal(A, B, C)]
    for P, Q in ((A, B), (B, C), (C, A)):
        d = [Q[i] - P[i] for i in range(3)]
        L += [cross(e, d) for e in units]
    return L


def touches_int(t, p):
    """the TOUCHED predicate for voxel p in Python integers"""
    tri = vertices(t)
    if tri is None:
        return False
    o = [UNIT * int(q) for q in p]
    for L in axes_of(*tri):
        base = sum(L[i] * o[i] for i in range(3))
        box_lo = base + UNIT * sum(min(q, 0) for q in L)
        box_hi = base + UNIT * sum(max(q, 0) for q in L)
        dots = [sum(L[i] * V[i] for i in range(3)) for V in tri]
        if box_lo > max(dots) or min(dots) > box_hi:
            return False
    return True


def touched_voxels(S, t):
    """(m, 3) int64: the voxels of an S^3 volume whose closed cube meets the closed triangle, in [x, y, z] order"""
    tri = vertices(t)
    if tri is None:
        return np.zeros((0, 3), np.int64)
    lo = [max(0, -((UNIT - min(V[i] for V in tri)) // UNIT)) for i in range(3)]          # ceil((min - 64) / 64)
    hi = [min(S - 1, max(V[i] for V in tri) // UNIT) for i in range(3)]
    if any(lo[i] > hi[i] for i in range(3)):
        return np.zeros((0, 3), np.int64)
    o = [UNIT * np.arange(lo[i], hi[i] + 1, dtype=np.int64).reshape([-1 if j == i else 1 for j in range(3)]) for i in range(3)]
    ok = np.ones([hi[i] - lo[i] + 1 for i in range(3)], bool)
    for L in axes_of(*tri):
        assert max(abs(q) for q in L) < 1 << 38
        base = np.int64(L[0]) * o[0] + np.int64(L[1]) * o[1] + np.int64(L[2]) * o[2]
        dots = [sum(L[i] * V[i] for i in range(3)) for V in tri]
        ok &= (base + np.int64(UNIT * sum(min(q, 0) for q in L)) <= np.int64(max(dots)))
        ok &= (np.int64(min(dots)) <= base + np.int64(UNIT * sum(max(q, 0) for q in L)))
    return np.argwhere(ok) + np.array(lo, np.int64)


_CENTRES = {}


def centres(S):
    if S not in _CENTRES:
        c = UNIT * np.arange(S, dtype=np.int64) + HALF
        _CENTRES[S] = (c[:, None], c[None, :])
    return _CENTRES[S]


def thin_voxels(S, t):
    """(m, 3) int64: per axis a, in every column (u, v) of the volume that the triangle's projection covers, the voxel that
    holds the crossing of the column's centre line with the plane, where it lies in the volume; duplicates are possible"""
    tri = vertices(t)
    if tri is None:
        return np.zeros((0, 3), np.int64)
    A, B, C = tri
    n = normal(A, B, C)
    cu, cv = centres(S)
    found = []
    for a in range(3):
        if n[a] == 0:
            continue
        u, v = (a + 1) % 3, (a + 2) % 3
        s = 1 if n[a] > 0 else -1
        an = abs(n[a])
        covered = np.ones((S, S), bool)
        for P, Q in ((A, B), (B, C), (C, A)):
            du, dv = s * (Q[u] - P[u]), s * (Q[v] - P[v])
            E = np.int64(du) * (cv - P[v]) - np.int64(dv) * (cu - P[u])
            covered &= (E > 0) | ((E == 0) & bool(dv > 0 or (dv == 0 and du < 0)))
        if not covered.any():
            continue
        M = np.int64(an) * np.int64(A[a]) - s * (np.int64(n[u]) * (cu - A[u]) + np.int64(n[v]) * (cv - A[v]))
        pa = M // np.int64(UNIT * an)                                  # floor
        iu, iv = np.nonzero(covered & (pa >= 0) & (pa < S))
        p = np.zeros((len(iu), 3), np.int64)
        p[:, a], p[:, u], p[:, v] = pa[iu, iv], iu, iv
        found.append(p)
    return np.concatenate(found) if found else np.zeros((0, 3), np.int64)


def selected(S, tris, mode):
    """(S, S, S) bool [x, y, z]: the voxels the (n, 9) triangles select"""
    sel = np.zeros((S, S, S), bool)
    one = touched_voxels if mode == TOUCHED else thin_voxels
    for t in np.asarray(tris).reshape(-1, 9):
        p = one(S, t)
        sel[p[:, 0], p[:, 1], p[:, 2]] = True
    return sel


def raster_mesh(S, tris, mode, solid=1, field=None):
    """field (S, S, S) uint8, the selected voxels all set or all cleared in place; a new empty field when None"""
    if field is None:
        field = np.zeros((S, S, S), np.uint8)
    field[selected(S, tris, mode)] = 1 if solid else 0
    return field


# ---- meshes the tests share ------------------------------------------------------------------------------------------

def box_mesh(lo, hi):
    """(12, 9) int64: the closed box with corners lo and hi (in units), two triangles a face, wound outwards"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    tris = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            q = np.zeros((4, 3), np.int64)
            for k, (du, dv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
                q[k, a] = hi[a] if side else lo[a]
                q[k, u] = hi[u] if du else lo[u]
                q[k, v] = hi[v] if dv else lo[v]
            order = [0, 1, 2, 0, 2, 3] if side else [0, 2, 1, 0, 3, 2]
            tris.append(q[order[:3]].reshape(9))
            tris.append(q[order[3:]].reshape(9))
    return np.array(tris, np.int64)


def corner_triangle(S):
    """the triangle (0,0,0) (S,S,0) (S,0,S) in voxels: it spans the volume corner to corner"""
    return np.array([[0, 0, 0, UNIT * S, UNIT * S, 0, UNIT * S, 0, UNIT * S]], np.int64)


def small_triangles(rng, S, count, reach=160):
    """(count, 9) int64 seeded triangles with edges of at most `reach` units around a volume of S^3, some a little outside, one
    in eight degenerate, one in eight on multiples of 32"""
    a = rng.integers(-UNIT, UNIT * S + UNIT, (count, 1, 3))
    t = a + np.concatenate([np.zeros((count, 1, 3), np.int64), rng.integers(-reach, reach + 1, (count, 2, 3))], axis=1)
    kind = rng.integers(0, 8, count)
    t[kind == 0, 2] = t[kind == 0, 1]
    t[kind == 1] = (t[kind == 1] // HALF) * HALF
    return t.reshape(count, 9)
