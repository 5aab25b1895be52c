"""numpy restatement of the rule of vrc_volume_extract_surface (include/vrc.h), the yardstick of the surface tests: which
faces of a voxel set are exposed, their canonical order, and their two triangles each.  tests/test_volume_surface_host.py
holds it against a per-voxel loop and against the voxeliser's model (the round trip)."""
import numpy as np

UNIT = 64                   # units per voxel, as vrc_volume_xor_mesh


def key_of(xyz, S):
    """the bit position of voxels (n, 3) in the occupancy of an S^3 volume: 8 * brick + (z&1) 4 + (y&1) 2 + (x&1)"""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    n = S // 2
    brick = ((x >> 1) * n + (y >> 1)) * n + (z >> 1)
    return 8 * brick + (z & 1) * 4 + (y & 1) * 2 + (x & 1)


def ordered(faces, S):
    """(n, 4) x y z d records in the canonical order: by occupancy word key >> 5, then d, then bit key & 31"""
    f = np.asarray(faces, np.int64).reshape(-1, 4)
    key = key_of(f[:, :3], S)
    return f[np.lexsort((key & 31, f[:, 3], key >> 5))].astype(np.uint32)


def faces(V, closed=True):
    """the exposed faces of the dense field V[x, y, z] (0 / 1), (n, 4) uint32 x y z d in the canonical order: face
    d = 2 * axis + side of a solid voxel is exposed iff its neighbour on that side is empty; beyond the volume lies
    emptiness (closed) or solid (open)"""
    V = np.asarray(V) != 0
    S = V.shape[0]
    assert V.shape == (S, S, S)
    P = np.pad(V, 1, constant_values=not closed)
    found = []
    for d in range(6):
        axis, side = d >> 1, d & 1
        window = [slice(1, S + 1)] * 3
        window[axis] = slice(2, S + 2) if side else slice(0, S)
        xyz = np.argwhere(V & ~P[tuple(window)])
        found.append(np.concatenate([xyz, np.full((xyz.shape[0], 1), d)], axis=1))
    return ordered(np.concatenate(found), S)


def triangles(face_records):
    """(2n, 9) int32: the two triangles of each face, in fixed point with 64 units per voxel, counter-clockwise seen from
    outside"""
    f = np.asarray(face_records, np.int64).reshape(-1, 4)
    n = f.shape[0]
    rows = np.arange(n)
    d = f[:, 3]
    a, s = d >> 1, d & 1
    u, v = (a + 1) % 3, (a + 2) % 3
    q = np.zeros((n, 4, 3), np.int64)
    for k, (du, dv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
        q[rows, k, a] = UNIT * (f[rows, a] + s)
        q[rows, k, u] = UNIT * (f[rows, u] + du)
        q[rows, k, v] = UNIT * (f[rows, v] + dv)
    out_plus = q[:, [0, 1, 2, 0, 2, 3], :]
    out_minus = q[:, [0, 2, 1, 0, 3, 2], :]
    return np.where((s == 1)[:, None, None], out_plus, out_minus).reshape(2 * n, 9).astype(np.int32)


def direction_counts(face_records):
    return np.bincount(np.asarray(face_records, np.int64).reshape(-1, 4)[:, 3], minlength=6).astype(np.uint64)


def word_direction_counts(face_records, S):
    """(words, 6) faces per occupancy word and direction: where the windows of the tests put their edges"""
    f = np.asarray(face_records, np.int64).reshape(-1, 4)
    out = np.zeros((S ** 3 // 32, 6), np.int64)
    np.add.at(out, (key_of(f[:, :3], S) >> 5, f[:, 3]), 1)
    return out
