"""numpy restatement of the rule of vrc_volume_xor_mesh (include/vrc.h), the yardstick of the voxelisation tests: int64
throughout, vectorised over a triangle's bounding box of voxel columns.  Fixed point with 6 fractional bits: the centre
of voxel (x, y, z) is (64x + 32, 64y + 32, 64z + 32).  tests/test_volume_voxelize_host.py holds it against boxes, a fan
and an exact orientation test of random tetrahedra."""
import numpy as np

FRAC = 6
UNIT = 1 << FRAC            # 64 units per voxel
HALF = UNIT // 2
LIMIT = 1 << 17             # a triangle with a coordinate beyond +-LIMIT is dropped


def xor_mesh(S, tris, field=None):
    """field (S, S, S) uint8 [x, y, z], XORed in place with the crossing parity of the (n, 9) integer triangles; a new
    empty field when None.  Returns the field."""
    if field is None:
        field = np.zeros((S, S, S), np.uint8)
    assert field.shape == (S, S, S) and field.dtype == np.uint8
    tris = np.asarray(tris).reshape(-1, 9)
    zs = np.arange(S, dtype=np.int64)
    for t in tris:
        c = [int(q) for q in t]
        if any(abs(q) > LIMIT for q in c):                    # Python ints: no wrap-around can hide an excess
            continue
        a, b, cc = c[0:3], c[3:6], c[6:9]
        u = [b[i] - a[i] for i in range(3)]
        w = [cc[i] - a[i] for i in range(3)]
        nx, ny, nz = u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]
        if nz == 0:
            continue
        s = 1 if nz > 0 else -1
        anz = abs(nz)
        assert max(abs(nx), abs(ny), anz) < 1 << 38
        # the columns whose centres lie in the xy bounding box, clipped to the volume
        x0 = max(0, -((HALF - min(a[0], b[0], cc[0])) // UNIT))        # ceil((min - 32) / 64)
        x1 = min(S - 1, (max(a[0], b[0], cc[0]) - HALF) // UNIT)
        y0 = max(0, -((HALF - min(a[1], b[1], cc[1])) // UNIT))
        y1 = min(S - 1, (max(a[1], b[1], cc[1]) - HALF) // UNIT)
        if x0 > x1 or y0 > y1:
            continue
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
        k = np.clip(-((-N) // D), 0, S)                        # ceil(N / D)
        flip = covered[:, :, None] & (zs[None, None, :] < k[:, :, None])
        field[x0:x1 + 1, y0:y1 + 1, :] ^= flip.astype(np.uint8)
    return field


def quantise(verts, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """(n, 3) float vertices -> int32 fixed point, each VERTEX once: rint((v * scale + offset) * 64) in float64"""
    v = np.asarray(verts, np.float64).reshape(-1, 3) * float(scale) + np.asarray(offset, np.float64).reshape(1, 3)
    return np.rint(v * UNIT).astype(np.int64).astype(np.int32)


def soup(verts_fixed, faces):
    """(n_faces, 9) triangles of integer vertices and (n_faces, 3) indices"""
    return np.asarray(verts_fixed)[np.asarray(faces, np.int64).reshape(-1, 3)].reshape(-1, 9).astype(np.int32)
