"""numpy restatement of the rule of vrc_volume_xor_mesh (include/vrc.h), the yardstick of the voxelisation tests: int64
throughout, vectorised over a triangle's bounding box of voxel columns.  Fixed point with 6 fractional bits: the centre
of voxel (x, y, z) is (64x + 32, 64y + 32, 64z + 32).  tests/test_volume_voxelize_host.py holds it against boxes, a fan
and an exact orientation test of random tetrahedra.  xor_mesh is the dense form; column_flips is the same rule per column,
sparse, for volumes of which nobody wants an S^3 array (tests/test_volume_voxelize_cases_host.py holds the two equal)."""
import numpy as np

FRAC = 6
UNIT = 1 << FRAC            # 64 units per voxel
HALF = UNIT // 2
LIMIT = 1 << 17             # a triangle with a coordinate beyond +-LIMIT is dropped


def triangle_columns(S, t, clamp=True):
    """One triangle (9 integers) in a volume of S^3: None where it contributes nothing (a coordinate beyond LIMIT, n.z == 0, no
    column centre in its bounding box), else (x0, y0, covered, k): the columns of its xy bounding box clipped to the volume
    start at (x0, y0); covered (nx, ny) bool [x, y]; k (nx, ny) int64 = clamp(ceil(N / D), 0, S), the column's flipped prefix
    [0, k) where covered.  clamp=False leaves a k above S as it is (for experiments with a wrong kernel)."""
    c = [int(q) for q in t]
    if any(abs(q) > LIMIT for q in c):                        # Python ints: no wrap-around can hide an excess
        return None
    a, b, cc = c[0:3], c[3:6], c[6:9]
    u = [b[i] - a[i] for i in range(3)]
    w = [cc[i] - a[i] for i in range(3)]
    nx, ny, nz = u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]
    if nz == 0:
        return None
    s = 1 if nz > 0 else -1
    anz = abs(nz)
    assert max(abs(nx), abs(ny), anz) < 1 << 38
    # the columns whose centres lie in the xy bounding box, clipped to the volume
    x0 = max(0, -((HALF - min(a[0], b[0], cc[0])) // UNIT))        # ceil((min - 32) / 64)
    x1 = min(S - 1, (max(a[0], b[0], cc[0]) - HALF) // UNIT)
    y0 = max(0, -((HALF - min(a[1], b[1], cc[1])) // UNIT))
    y1 = min(S - 1, (max(a[1], b[1], cc[1]) - HALF) // UNIT)
    if x0 > x1 or y0 > y1:
        return None
    px = (UNIT * np.arange(x0, x1 + 1, dtype=np.int64) + HALF)[:, None]
    py = (UNIT * np.arange(y0, y1 + 1, dtype=np.int64) + HALF)[None, :]
    covered = np.ones((x1 - x0 + 1, y1 - y0 + 1), bool)
    for P, Q in ((a, b), (b, cc), (cc, a)):
        dx, dy = s * (Q[0] - P[0]), s * (Q[1] - P[1])
        E = np.int64(dx) * (py - P[1]) - np.int64(dy) * (px - P[0])
        covered &= (E > 0) | ((E == 0) & bool(dy > 0 or (dy == 0 and dx < 0)))
    base = np.int64(nx) * (px - a[0]) + np.int64(ny) * (py - a[1])
    N = np.int64(anz) * np.int64(a[2] - HALF) - s * base
    D = np.int64(UNIT * anz)
    k = np.maximum(-((-N) // D), 0)                            # ceil(N / D)
    return x0, y0, covered, np.minimum(k, S) if clamp else k


def column_exact(S, t, x, y):
    """triangle_columns for ONE column in Python integers: None where the triangle does not cover the centre of column (x, y),
    else (k, the largest magnitude among N, N + D and the edge functions) -- the recheck of the rule where its products
    are largest"""
    c = [int(q) for q in t]
    if any(abs(q) > LIMIT for q in c):
        return None
    a, b, cc = c[0:3], c[3:6], c[6:9]
    u = [b[i] - a[i] for i in range(3)]
    w = [cc[i] - a[i] for i in range(3)]
    nx, ny, nz = u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]
    if nz == 0:
        return None
    s = 1 if nz > 0 else -1
    anz = abs(nz)
    px, py = UNIT * int(x) + HALF, UNIT * int(y) + HALF
    if not (min(a[0], b[0], cc[0]) <= px <= max(a[0], b[0], cc[0]) and min(a[1], b[1], cc[1]) <= py <= max(a[1], b[1], cc[1])):
        return None
    largest = 0
    for P, Q in ((a, b), (b, cc), (cc, a)):
        dx, dy = s * (Q[0] - P[0]), s * (Q[1] - P[1])
        E = dx * (py - P[1]) - dy * (px - P[0])
        largest = max(largest, abs(E))
        if not (E > 0 or (E == 0 and (dy > 0 or (dy == 0 and dx < 0)))):
            return None
    N = anz * (a[2] - HALF) - s * (nx * (px - a[0]) + ny * (py - a[1]))
    D = UNIT * anz
    return min(max(-((-N) // D), 0), S), max(largest, abs(N), abs(N) + D)


def reduced(S, rows):
    """(m, 3) int64 rows (x, y, k) modulo two: a row that occurs an even number of times and every row with k == 0 is left out;
    the rest once each, sorted by (x, y, k)"""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    rows = rows[rows[:, 2] > 0]
    key, count = np.unique((rows[:, 0] * S + rows[:, 1]) * (S + 1) + rows[:, 2], return_counts=True)
    key = key[count % 2 == 1]
    return np.stack([key // (S + 1) // S, key // (S + 1) % S, key % (S + 1)], axis=1)


def column_flips(S, tris):
    """The sparse form of xor_mesh on an empty field: (m, 3) int64 rows (x, y, k), reduced -- column (x, y) is flipped on
    [0, k) once per row, so voxel z of a column is flipped iff an odd number of the column's rows have k > z.  No S^3 array."""
    rows = []
    for t in np.asarray(tris).reshape(-1, 9):
        cols = triangle_columns(S, t)
        if cols is None:
            continue
        x0, y0, covered, k = cols
        ix, iy = np.nonzero(covered)
        rows.append(np.stack([ix + x0, iy + y0, k[ix, iy]], axis=1))
    return reduced(S, np.concatenate(rows) if rows else np.zeros((0, 3), np.int64))


def runs_of_flips(flips):
    """(r, 4) int64 rows (x, y, z0, z1) of reduced flips: the runs [z0, z1) of each column that are flipped an odd number of
    times, ascending within a column.  From the top: [k_(m-1), k_m), [k_(m-3), k_(m-2)), ... with k_0 = 0"""
    flips = np.asarray(flips, np.int64).reshape(-1, 3)
    if not len(flips):
        return np.zeros((0, 4), np.int64)
    first = np.concatenate([[True], (flips[1:, :2] != flips[:-1, :2]).any(axis=1)])      # rows are sorted by (x, y, k)
    start = np.flatnonzero(first)
    size = np.diff(np.concatenate([start, [len(flips)]]))                # rows per column
    index = np.arange(len(flips)) - np.repeat(start, size)
    top = (np.repeat(size, size) - 1 - index) % 2 == 0
    below = np.where(first, 0, np.concatenate([[0], flips[:-1, 2]]))
    return np.stack([flips[top, 0], flips[top, 1], below[top], flips[top, 2]], axis=1)


def count_of_flips(flips):
    """the number of voxels the reduced flips change"""
    runs = runs_of_flips(flips)
    return int((runs[:, 3] - runs[:, 2]).sum())


def dense_of_flips(S, flips, field=None):
    """field (S, S, S) uint8 [x, y, z] XORed in place with reduced flips; a new empty field when None"""
    if field is None:
        field = np.zeros((S, S, S), np.uint8)
    flips = np.asarray(flips, np.int64).reshape(-1, 3)
    marks = np.zeros((S, S, S + 1), np.uint8)
    marks[flips[:, 0], flips[:, 1], flips[:, 2]] = 1                     # reduced: every row once
    field ^= np.bitwise_xor.accumulate(marks[:, :, :0:-1], axis=2)[:, :, ::-1]      # z flips iff an odd number of k > z
    return field


def xor_mesh(S, tris, field=None):
    """field (S, S, S) uint8 [x, y, z], XORed in place with the crossing parity of the (n, 9) integer triangles; a new
    empty field when None.  Returns the field."""
    if field is None:
        field = np.zeros((S, S, S), np.uint8)
    assert field.shape == (S, S, S) and field.dtype == np.uint8
    zs = np.arange(S, dtype=np.int64)
    for t in np.asarray(tris).reshape(-1, 9):
        cols = triangle_columns(S, t)
        if cols is None:
            continue
        x0, y0, covered, k = cols
        flip = covered[:, :, None] & (zs[None, None, :] < k[:, :, None])
        field[x0:x0 + covered.shape[0], y0:y0 + covered.shape[1], :] ^= flip.astype(np.uint8)
    return field


def quantise(verts, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """(n, 3) float vertices -> int32 fixed point, each VERTEX once: rint((v * scale + offset) * 64) in float64"""
    v = np.asarray(verts, np.float64).reshape(-1, 3) * float(scale) + np.asarray(offset, np.float64).reshape(1, 3)
    return np.rint(v * UNIT).astype(np.int64).astype(np.int32)


def soup(verts_fixed, faces):
    """(n_faces, 9) triangles of integer vertices and (n_faces, 3) indices"""
    return np.asarray(verts_fixed)[np.asarray(faces, np.int64).reshape(-1, 3)].reshape(-1, 9).astype(np.int32)
