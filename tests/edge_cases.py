"""Ray batches at the edges of the per-ray operators' inputs (include/vrc.h: vrc_grid_cast_rays, vrc_cast_ray_chains) and the
one relaxed comparison they need.  Inputs only: the same arrays go to the oracle and to the kernel.  Shared by
tests/test_gpu_grid.py, tests/test_gpu_chains.py and tests/tools/fuzz_gpu.py --chains."""
import numpy as np

import raygen

F = np.float32
FLOAT_FIELDS = ["position", "normal", "voxel_coord", "distance"]
FIELDS = ["position", "normal", "voxel_coord", "hit", "node", "distance", "complexity"]
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(1e-45)           # 2^-149


def assert_hits_equal_nan_relaxed(got, ref):
    """Every field as uint32, as test_gpu_cast.assert_hits_equal compares them, with one exception: a float that is NaN on
    both sides counts as equal.  (A zero direction in a solid grid is a hit at org + inf * 0 in the reference: the hardware
    fixes the sign and payload of that NaN, not the algorithm.)  Returns (lanes compared relaxed, lanes whose oracle record
    holds a NaN); the relaxed lanes are a subset of the latter by assertion."""
    assert got.shape == ref.shape
    n = len(ref)
    ref_nan = np.zeros(n, bool)
    relaxed = np.zeros(n, bool)
    for f in FIELDS:
        x = np.ascontiguousarray(got[f]).view(np.uint32).reshape(n, -1)
        y = np.ascontiguousarray(ref[f]).view(np.uint32).reshape(n, -1)
        differ = x != y
        if f in FLOAT_FIELDS:
            gn = np.isnan(np.ascontiguousarray(got[f]).reshape(n, -1))
            rn = np.isnan(np.ascontiguousarray(ref[f]).reshape(n, -1))
            ref_nan |= rn.any(1)
            both = gn & rn
            relaxed |= (differ & both).any(1)
            differ &= ~both
        if differ.any():
            bad = np.flatnonzero(differ.any(1))
            raise AssertionError(f"field {f}: {len(bad)} of {n} rays differ, first {bad[:5]}: {got[bad[0]]} vs {ref[bad[0]]}")
    assert not (relaxed & ~ref_nan).any()
    return int(relaxed.sum()), int(ref_nan.sum())


# ---- dense grid ----------------------------------------------------------------------------------------------------------

def grid_cells(shape, density, seed=0):
    if density >= 1.0:
        return np.ones(shape, np.uint8)
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def sample_directions(rng, k=8):
    """the six axis directions, the eight diagonals and k random ones"""
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    diag = [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    return np.concatenate([np.asarray(axes + diag, F), rng.normal(size=(k, 3)).astype(F)])


def cross(org, d):
    """every origin with every direction"""
    org, d = np.asarray(org, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    return np.repeat(org, len(d), axis=0), np.tile(d, (len(org), 1))


def per_component_and_all(base, values):
    """base (3,) with each value in each component separately and in all three"""
    out = []
    for v in values:
        for a in range(3):
            o = np.array(base, F)
            o[a] = v
            out.append(o)
        out.append(np.full(3, v, F))
    return np.asarray(out, F)


def grid_origin_non_finite(shape, rng):
    """NaN, +-inf and values outside the int32 range as origin coordinates: rays that start nowhere"""
    vals = [np.nan, -np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 3e9, -3e9, FLT_MAX, -FLT_MAX]
    base = (np.asarray(shape, F) * F(0.5) + F(0.25)).astype(F)
    org = np.concatenate([per_component_and_all(base, vals), per_component_and_all(np.asarray([0.5, 0.5, 0.5], F), vals)])
    nan_payload = np.asarray([0x7fc00001, 0xffc00000, 0x7f800001, 0xffffffff], np.uint32).view(F)     # quiet, signalling
    org = np.concatenate([org, per_component_and_all(base, nan_payload)])
    return cross(org, sample_directions(rng))


def grid_direction_edges(shape, rng):
    """NaN, +-inf, +-0, denormal, smallest-normal and 2^127 direction components"""
    vals = [np.nan, np.inf, -np.inf, 0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1e-40, -1e-40, 2.0 ** -126, -2.0 ** -126,
            2.0 ** 127, -2.0 ** 127]
    d = np.concatenate([per_component_and_all(b, vals) for b in ([0.3, -0.7, 0.64], [-1.0, 1.0, 1.0], [0.0, 0.0, 1.0])])
    sh = np.asarray(shape, F)
    org = np.concatenate([(rng.random((12, 3)) * sh).astype(F), np.floor(rng.random((4, 3)) * sh).astype(F),
                          [np.zeros(3, F), sh * F(0.5)]])
    return cross(org, d)


def grid_boundary_origins(shape, rng):
    """origins exactly on every integer plane (0 and X, Y, Z included), in (-1, 0) and [X, X + 1), and one cell outside each
    face pointing inwards.  Returns (org, dir, must_miss): the lanes that start outside the grid, which the reference misses."""
    sh = np.asarray(shape, F)
    inside = (rng.random((4, 3)) * sh).astype(F)
    org = []
    for a in range(3):
        for p in range(int(shape[a]) + 1):                    # on the planes of one axis ...
            for b in inside:
                o = b.copy()
                o[a] = p
                org.append(o)
            org.append(np.minimum(np.full(3, p, F), sh))       # ... and of all three
    for a in range(3):                                         # truncation towards zero: (-1, 0) is cell 0, [X, X + 1) is outside
        for v in (-0.5, -1e-3, -0.999, -float(DENORM_MIN), -0.0, -1.0, -1.5, -2.0):
            for b in inside[:2]:
                o = b.copy()
                o[a] = v
                org.append(o)
        for v in (0.0, 1e-3, 0.5, 0.999, 1.0, 1.5):
            for b in inside[:2]:
                o = b.copy()
                o[a] = sh[a] + F(v)
                org.append(o)
    for v in (-0.5, -1e-3):
        org.append(np.full(3, v, F))
    org = np.asarray(org, F)
    o, d = cross(org, sample_directions(rng, 4))
    # one cell outside each face, pointing straight and obliquely inwards
    fo, fd = [], []
    for a in range(3):
        for side in (0, 1):
            for b in inside:
                o1 = b.copy()
                o1[a] = -1.5 if side == 0 else sh[a] + F(0.5)
                for tilt in (0.0, 0.3):
                    d1 = np.full(3, tilt, F)
                    d1[a] = 1.0 if side == 0 else -1.0
                    fo.append(o1)
                    fd.append(d1)
    o, d = np.concatenate([o, np.asarray(fo, F)]), np.concatenate([d, np.asarray(fd, F)])
    cell = np.trunc(o)
    must_miss = ((cell < 0) | (cell >= sh)).any(1)
    return o, d, must_miss


def grid_inside_rays(shape, rng, n):
    sh = np.asarray(shape, F)
    org = (rng.random((n, 3)) * sh).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    k = n // 8
    for a in range(3):
        d[a * k:(a + 1) * k] = 0
        d[a * k:(a + 1) * k, a] = rng.choice([-1.0, 1.0], k).astype(F)
    return org, d


# ---- chains of two casts ---------------------------------------------------------------------------------------------------

CHAIN_KINDS = ["next_to_hit", "random", "outside_and_planes", "non_finite", "same_as_a"]


def chain_rays_a(depth, n, rng, targets=None, camera_at=None):
    """Ray A: camera-like rays and random rays from inside [1, 2)^3, rays aimed at `targets` (points in [1, 2)^3) where the
    scene is too sparse to be hit by chance, and a share of guaranteed misses (pointing out of the cube from outside it, or
    passing it by).  camera_at: the camera's position in the cube's coordinates (raygen.camera_rays puts it at the BASELINE
    height 200 S / 512, which is inside the terrain's solid band for S < 512: every ray a hit at t = 0 without a normal)."""
    parts_o, parts_d = [], []
    q = max(n // 4, 1)
    W = max(int(np.sqrt(q * 16 / 9)), 1)
    H = max(q // W, 1)
    o, d = raygen.camera_rays(depth, W, H, float(rng.uniform(-1.2, -0.2)))
    if camera_at is not None:
        o = np.broadcast_to(np.asarray(camera_at, F), o.shape).copy()
    parts_o.append(o)
    parts_d.append(d)
    o = rng.uniform(1.0, 2.0, (q, 3)).astype(F)
    if targets is not None:
        d = (targets[rng.integers(0, len(targets), q)] - o).astype(F)
    else:
        d = rng.normal(size=(q, 3)).astype(F)
    parts_o.append(o)
    parts_d.append(d)
    o, d = raygen.mixed_rays(max(q, 16), int(rng.integers(1 << 30)))       # axis-parallel, +-0 and tiny components, non-unit ...
    parts_o.append(rng.uniform(1.0, 2.0, (q, 3)).astype(F))                # ... from inside the cube: a hit on the cube's own
    parts_d.append(d[:q])                                                  # faces has no neighbour cell to start B in
    org, d = np.concatenate(parts_o), np.concatenate(parts_d)
    m = n - len(org)
    if m > 0:                                                  # misses: outside the cube, pointing away from it
        o = rng.uniform(2.0, 3.0, (m, 3)).astype(F)
        dd = np.abs(rng.normal(size=(m, 3))).astype(F) + F(0.01)
        flip = rng.random(m) < 0.5
        o[flip] = (F(3.0) - o[flip]).astype(F)
        dd[flip] = -dd[flip]
        org, d = np.concatenate([org, o]), np.concatenate([d, dd])
    p = rng.permutation(len(org))[:n]
    return np.ascontiguousarray(org[p], F), np.ascontiguousarray(d[p], F)


def _normalize(v):
    v = v.astype(F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return (v / np.sqrt((v * v).sum(1, dtype=F)).astype(F)[:, None]).astype(F)


def chain_rays_b(kind, depth, org_a, dir_a, ref_a, light, rng):
    """Ray B of one kind for every ray A, given A's hits (the oracle's)."""
    n = len(org_a)
    hit = ref_a["hit"] != 0
    inv_size = F(1.0) / F(1 << depth)
    # raycaster.hpp:139,153 -- the frame kernels' own secondary ray: next to the hit along its normal, towards the light;
    # where A missed, any ray
    next_o = (ref_a["position"] + ref_a["normal"] * (inv_size * F(0.001))).astype(F)
    next_o[~hit] = rng.uniform(1.0, 2.0, (int((~hit).sum()), 3)).astype(F)
    next_d = _normalize(np.asarray(light, F)[None, :] - next_o)
    if kind == "next_to_hit":
        return next_o, next_d
    if kind == "random":
        d = rng.normal(size=(n, 3)).astype(F)
        d[::5] *= F(9.0)
        return rng.uniform(1.0, 2.0, (n, 3)).astype(F), d
    if kind == "outside_and_planes":
        o = next_o.copy()
        d = np.where(rng.random((n, 1)) < 0.5, next_d, rng.normal(size=(n, 3))).astype(F)
        third = n // 3
        o[:third] = rng.uniform(0.0, 3.0, (third, 3)).astype(F)                 # mostly outside [1, 2)^3
        far = slice(0, third, 7)
        o[far] = (o[far] * F(1000.0) - F(1500.0)).astype(F)
        rest = np.arange(third, n)                                              # exactly 1.0, 1.5, 2.0 on one to three axes
        k = rng.integers(1, 4, len(rest))
        val = rng.choice(np.asarray([1.0, 1.5, 2.0], F), (len(rest), 3))
        order = np.argsort(rng.random((len(rest), 3)), axis=1)
        on = order < k[:, None]
        base = np.where(rng.random((len(rest), 1)) < 0.5, o[rest], rng.uniform(1.0, 2.0, (len(rest), 3))).astype(F)
        o[rest] = np.where(on, val, base)
        return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    if kind == "non_finite":
        o, d = next_o.copy(), next_d.copy()
        vals = np.asarray([np.nan, np.inf, -np.inf], F)
        i = np.arange(n)
        which = rng.integers(0, 3, n)                      # 0: origin, 1: direction, 2: left finite (the neighbours of a bad lane)
        axis = rng.integers(0, 3, n)
        v = vals[rng.integers(0, 3, n)]
        so, sd = which == 0, which == 1
        o[i[so], axis[so]] = v[so]
        d[i[sd], axis[sd]] = v[sd]
        allthree = rng.random(n) < 0.1
        o[so & allthree] = v[so & allthree, None]
        d[sd & allthree] = v[sd & allthree, None]
        return o, d
    if kind == "same_as_a":
        return org_a.copy(), dir_a.copy()
    raise ValueError(kind)


def carved_volume(depth, rng):
    """a random volume with spheres carved out of it and one added (leaves at every level)"""
    S0 = 1 << depth
    g = np.indices((S0, S0, S0)).astype(np.float32)
    vol = rng.random((S0, S0, S0)) < 0.35
    for k in range(4):
        c, r = rng.uniform(0, S0, 3), rng.uniform(S0 / 8, S0 / 2.5)
        ball = ((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) < r * r
        vol = (vol | ball) if k == 3 else (vol & ~ball)
    if not vol.any():
        vol[0, 0, 0] = True
    return vol.astype(np.uint8)


CHAIN_COEFS = (0.0, 0.25, 0.5)
CHAIN_SIZES = (1, 255, 256, 257)           # ... and the whole batch


def gpu_chain_caster(svo):
    """cast(org_a, dir_a, org_b, dir_b, coef_b, want_not_executed) -> (out_a, out_b, not_executed or None) through
    vrc_cast_ray_chains on device buffers.  The outputs are filled with 0xAB first: every lane has to be written."""
    import torch
    import cpuvoxelraycaster_amd as vrc

    def cast(org_a, dir_a, org_b, dir_b, coef_b, want_not_executed=True):
        n = len(org_a)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, F).reshape(-1)).cuda()
        d_oa, d_da, d_ob, d_db = t(org_a), t(dir_a), t(org_b), t(dir_b)
        out_a = torch.full((n * 48,), 0xAB, dtype=torch.uint8, device="cuda")
        out_b = torch.full((n * 48,), 0xAB, dtype=torch.uint8, device="cuda")
        skipped = torch.full((n,), -1, dtype=torch.int32, device="cuda") if want_not_executed else None
        torch.cuda.synchronize()
        svo.castRayChainsDevice(n, d_oa.data_ptr(), d_da.data_ptr(), d_ob.data_ptr(), d_db.data_ptr(), coef_b, out_a.data_ptr(),
                                out_b.data_ptr(), skipped.data_ptr() if want_not_executed else None)
        torch.cuda.synchronize()
        a = np.frombuffer(out_a.cpu().numpy().tobytes(), dtype=vrc.HIT_DTYPE)
        b = np.frombuffer(out_b.cpu().numpy().tobytes(), dtype=vrc.HIT_DTYPE)
        return a, b, (skipped.cpu().numpy().view(np.uint32) if want_not_executed else None)
    return cast


def first_difference(got, ref):
    differ = (got.view(np.uint8).reshape(len(ref), -1) != ref.view(np.uint8).reshape(len(ref), -1)).any(axis=1)
    return int(differ.sum()), np.flatnonzero(differ)[:5]


def check_chains(cast, cast_oracle, depth, kind, org_a, dir_a, light, rng):
    """The contract of vrc_cast_ray_chains (include/vrc.h) for one kind of ray B on one scene, strict comparison throughout:
    out_a = the oracle's cast of A; out_b = the oracle's cast of B alone with coef_b, complexity included; not_executed is 0
    where A missed and at most depth - 1 anywhere; NULL for not_executed changes nothing.  For every coefficient of
    CHAIN_COEFS, on the whole batch and on its first 1, 255, 256, 257 chains.  cast_oracle(org, dir, coef) is O.cast_rays on
    the scene.  Returns the figures it looked at."""
    n = len(org_a)
    ref_a = cast_oracle(org_a, dir_a, 0.0)
    hit_a = ref_a["hit"] != 0
    org_b, dir_b = chain_rays_b(kind, depth, org_a, dir_a, ref_a, light, rng)
    finite_b = np.isfinite(org_b).all(1) & np.isfinite(dir_b).all(1)
    stats = dict(n=n, hits_a=int(hit_a.sum()), non_finite_b=int((~finite_b).sum()))
    for coef in CHAIN_COEFS:
        ref_b = cast_oracle(org_b, dir_b, coef)
        assert not ref_b["hit"][~finite_b].any() and not ref_b["complexity"][~finite_b].any()
        for m in CHAIN_SIZES + (n,):
            if m > n:
                continue
            got_a, got_b, skipped = cast(org_a[:m], dir_a[:m], org_b[:m], dir_b[:m], coef, True)
            bad, first = first_difference(got_a, ref_a[:m])
            assert not bad, f"out_a: {bad} of {m} differ (coef {coef}), first {first}: {got_a[first[0]]} vs {ref_a[first[0]]}"
            bad, first = first_difference(got_b, ref_b[:m])
            assert not bad, (f"out_b: {bad} of {m} differ (coef {coef}, kind {kind}), first {first}: org {org_b[first[0]].tolist()} "
                             f"dir {dir_b[first[0]].tolist()} A's hit {ref_a[first[0]]}: {got_b[first[0]]} vs {ref_b[first[0]]}")
            assert not skipped[~hit_a[:m]].any()
            assert int(skipped.max()) <= depth - 1
            assert not skipped[~finite_b[:m]].any()
            if m in (257, n):
                null_a, null_b, _ = cast(org_a[:m], dir_a[:m], org_b[:m], dir_b[:m], coef, False)
                assert null_a.tobytes() == got_a.tobytes() and null_b.tobytes() == got_b.tobytes()
        stats[f"started_below_{coef}"] = float((skipped[hit_a] > 0).mean()) if hit_a.any() else 0.0
        if kind == "next_to_hit":           # the path under test ran
            assert (skipped[hit_a] > 0).mean() > 0.5, stats
    stats["hits_b"] = int((ref_b["hit"] != 0).sum())
    return stats
