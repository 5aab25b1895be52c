"""Seeded programs of mixed calls on ONE long-lived pair of volumes, and their numpy mirror: what
tests/test_gpu_volume_program.py runs on the device and tests/test_volume_program_host.py holds to its purpose on the CPU.
numpy and Python integers only; every expected value comes from the model the family's own tests use (stamp_model,
flood_model, cells_model, delta_model, pack_model, voxelize_model, surface_model, rect_model, components_model,
distance_model, fall_model, stroke_model, raster_model, columns_model, voxels_model); the sphere predicate is vrc.h:208-210 taken literally,
as the brushes' tests take it.

A step is (family, form, arguments): a plain record.  `v` is the program's volume, `w` the second one.

Forms: "host" = host memory (synchronous); "dev0" = device memory on the NULL stream; "devA" / "devB" = device memory on
the first / second stream of the test's own.  A family without a memory kind (copyRegion, stampAffine, fillRandom,
applyDelta, cellStep, selectColumns) takes only the stream from its form.  rasterMesh keeps its mode under the key "op", so
that the tour takes both modes as it takes every op; voxels keeps its `which` there for the same reason.  listToSecond (the
x y z list of `v` extracted into device memory and set in `w` from there, on one stream) has no host form at all.

ORDERING says, per combination of a call with what may still be in flight, who orders it.  The GPU test downloads both
volumes after EVERY step, and vrc_volume_download is "synchronous, after every edit issued so far" (vrc.h:191-192), so
between two steps nothing is in flight: every two-stream combination between steps is synchronised by the program, as
vrc.h:178-179 asks of a caller ("issue a volume's asynchronous edits on ONE stream (or order the streams yourself)").  The
combinations INSIDE a step are the library's to order: the download right behind a device-memory edit (vrc.h:191-192), the
host-memory list call or query that a brush or a stroke at hits carries in its `then` argument (vrc.h:205-206, 219-220 and,
for the stroke, 249-250: the centres lie in the staging block, in flight on the caller's stream, and the stroke's kernel
reads centre i and i + 1 there), and the synchronous surface / rectangle / voxel count issued while a
device-memory extraction of the same step is still on its stream (order "extract_first"; vrc.h:350-351, 394-395, 444-447).
The voxel lists keep no block of their own: they use the surface calls' offsets block (vrc.h:454-455), so a count of EITHER
family behind an extraction of the other is the library's to order as well (orders "surface_behind", "voxels_behind").

Sizes of the per-volume scratch blocks (Mirror.scratch_bytes), each restated with the place it was read off (the StagePart
lists of the entry points in vrc_volume.hip, by function):
  staging, host form   12 n set_voxels, 24 n fill_boxes, 16 n fill_spheres, 64 n brush at hits, 16 n in device form (hits_call),
                       36 n xor_mesh, 13 n get_voxels, 32 n count_boxes, 16 per face / rectangle of a host window
                       (mesh_extract), 32 n fill_capsules, 64 n stroke at hits, 16 n in device form (hits_call), 36 n raster_mesh,
                       record * min(window, 2^20) of a host voxel list, record = 12 (x y z) or 16 (x y z m) and
                       window = window_of(first, capacity, T); nothing where the window is empty (windowed_extract)
  column calls         nothing: the 16 U V records of a host profile and the 4 U V bytes of each host map of a fill are
                       staged in a block of the call's own (vrc.h:1329-1330; volume_call in vrc_volume_state.h gives these
                       calls stage_in_v = false, vrc_columns_profile and vrc_columns_fill size the parts), and
                       vrc_columns_select stages nothing
  mark field           8^(depth-1) (vrc_voxelize.hip:145)
  surface offsets      8 (ceil(8^depth / 32 / 256) + 7) (vrc_surface.hip, surface_scratch_bytes); the voxel lists use the same block and add
                       nothing (reserve_voxel_slots in vrc_volume.hip); a refused voxel call reserves nothing (vrc_voxels_extract checks first)
  rectangle block      8 (ceil(6 S^2 w / 256) + 7) + 8 S^2 w, w = max(1, S / 32) (vrc_rects.hip, rect_scratch_bytes)
  pack slots           64 + 8 (tiles + 1) (vrc_pack.hip:327)
  flood block          4 (3 T^3 + 8), T = max(1, S / 32) (vrc_flood.hip:186-190), on the REGION
"""
import functools

import numpy as np

import cells_model
import columns_model
import components_model
import delta_model
import distance_model
import fall_model
import flood_model
import pack_model
import raster_model
import rect_model
import stamp_model
import stroke_model
import surface_model
import voxelize_model
import voxels_model

REPLACE, OR, ANDNOT = 0, 1, 2
TOUCHED, THIN = raster_model.TOUCHED, raster_model.THIN
FORMS = ("host", "dev0", "devA", "devB")
HIT_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("voxel_coord", "<f4", 2), ("hit", "<u4"), ("node", "<u4"),
                      ("distance", "<f4"), ("complexity", "<u4")])                  # vrc_hit, 48 bytes (include/vrc.h)

DEPTHS = (2, 3, 5, 6)
SEEDS = {2: (21, 22, 23), 3: (31, 32, 33), 5: (51, 52, 53), 6: (61, 62, 63)}
STEPS = {2: 232, 3: 232, 5: 232, 6: 130}
GUARD = 0x5A5A5A5A                                                     # what a device buffer of the test's own holds where nothing was written
COMMITTED = [(seed, depth) for depth in DEPTHS for seed in SEEDS[depth]]

ORDERING = {
    # (what runs, what may be in flight): (who orders it, where it says so)
    ("download", "device-memory edit of the same step"): ("library", "vrc.h:191-192"),
    ("then: host list call / query", "brush at hits of the same step"): ("library", "vrc.h:205-206, 219-220"),
    ("then: host list call / query", "stroke at hits of the same step, its kernel reading centres i and i + 1"): ("library", "vrc.h:249-250"),
    ("surface / rect count", "device-memory extraction of the same step (order extract_first)"): ("library", "vrc.h:350-351, 394-395"),
    ("voxel count of another which", "device-memory voxel extraction of the same step (order extract_first)"): ("library", "vrc.h:444-447"),
    ("surface count", "device-memory voxel extraction of the same step, in the block they share (order surface_behind)"): ("library", "vrc.h:350-351, 444-447, 454-455"),
    ("voxel count", "device-memory surface extraction of the same step, in the block they share (order voxels_behind)"): ("library", "vrc.h:350-351, 444-447, 454-455"),
    ("setVoxelsDevice into w", "device-memory voxel extraction from v of the same step, on the same stream (listToSecond)"): ("caller: one stream", "vrc.h:439-440"),
    ("listToSecond on one stream", "an edit of v of the step before, on the other stream"): ("program: the download between the steps", "vrc.h:178-179, 191-192"),
    ("any call", "an edit of an earlier step, on any stream"): ("program: the download between the steps", "vrc.h:178-179, 191-192"),
}

LIST_EDITS = ("setVoxels", "fillBoxes", "fillSpheres", "fillSpheresAtHits", "xorMesh", "fillCapsules", "strokeAtHits", "rasterMesh")
STREAM_EDITS = ("copyRegion", "stampAffine", "fillRandom", "applyDelta", "cellStepDst", "cellStepSrc", "selectColumnsDst", "selectColumnsSrc")
OTHER_EDITS = ("unpack", "floodRegion", "floodMedium", "keepConnected", "dilate", "erode", "select", "place", "fillColumns", "listToSecond")
EDITS = LIST_EDITS + STREAM_EDITS + OTHER_EDITS
QUERIES = ("solidCount", "getVoxels", "countBoxes", "surface", "rects", "pack", "diff", "components", "distanceAt", "commit", "columnProfile", "voxels")
REFUSALS = ("refuseOp", "refusePack", "refuseUnpack", "refuseDelta", "refuseDepth", "refuseMesh", "refuseRaster", "refuseStroke", "refuseProfile",
            "refuseFillAxis", "refuseSelect", "refuseSelectSame", "refuseSelectDepth", "refuseVoxels", "refuseVoxelsAligned")
AT_HITS = ("fillSpheresAtHits", "strokeAtHits")                       # the centres pass through the staging block in every form
LIFETIME = ("cloneSecond", "recreateSecond", "snapshotLabels", "snapshotClone")
FAMILIES = EDITS + QUERIES + REFUSALS + LIFETIME

# the families that share a persistent block of `v` (struct vrc_volume in vrc_volume_state.h); d_stage: in a form that stages
BLOCKS = {
    "d_stage": ("setVoxels", "fillBoxes", "fillSpheres", "fillSpheresAtHits", "xorMesh", "getVoxels", "countBoxes", "surface", "rects",
                "fillCapsules", "strokeAtHits", "rasterMesh", "voxels"),
    "d_marks": ("xorMesh",),
    "d_flood": ("floodRegion",),
    "d_surface": ("surface", "voxels", "listToSecond"),
    "d_rects": ("rects",),
    "d_pack": ("pack", "unpack", "refusePack", "refuseUnpack"),
    "grids": ("commit",),
    "d_count": ("solidCount", "floodRegion"),
}
# the host forms of these stage in a block of the call's own (vrc.h:1329-1330): they sit next to the users of d_stage, and leave it alone
OWN_BLOCK = ("columnProfile", "fillColumns")
FAULTS = ("marks", "stage_tail", "rows", "commit", "unordered", "links", "totals")
EDITS_OF_W = ("floodMedium", "cellStepSrc", "selectColumnsSrc", "listToSecond")


def stages(step):
    """the step writes v's staging block"""
    family, form, _ = step
    return family in BLOCKS["d_stage"] and (form == "host" or family in AT_HITS)


def shared_pairs():
    """every (block, A, B): an ordered pair of families that share the block"""
    return sorted((block, a, b) for block, users in BLOCKS.items() for a in users for b in users)


def covers(previous, step):
    """the (block, A, B) that two adjacent steps cover; for d_stage both must be in a form that writes the block"""
    return {(block, previous[0], step[0]) for block, users in BLOCKS.items()
            if previous[0] in users and step[0] in users and (block != "d_stage" or (stages(previous) and stages(step)))}


# ---- the sizes ---------------------------------------------------------------------------------------------------

def marks_bytes(depth):
    return 8 ** (depth - 1)


def surface_bytes(depth):
    return 8 * ((8 ** depth // 32 + 255) // 256 + 7)


def rects_bytes(depth):
    S = 1 << depth
    w = max(1, S // 32)
    return 8 * ((6 * S * S * w + 255) // 256 + 7) + 8 * S * S * w


def pack_bytes(depth):
    return 64 + 8 * (pack_model.Shape(depth).NT + 1)


def flood_bytes(depth):
    T = max(1, (1 << depth) // 32)
    return 4 * (3 * T ** 3 + 8)


ITEM_BYTES = {"setVoxels": 12, "fillBoxes": 24, "fillSpheres": 16, "xorMesh": 36, "getVoxels": 13, "countBoxes": 32, "fillCapsules": 32,
              "rasterMesh": 36}


# ---- small models ------------------------------------------------------------------------------------------------

def spheres(vol, items, value):
    """vrc.h:208-210: (x-cx)^2 + (y-cy)^2 + (z-cz)^2 <= r^2 in integers, clipped; r < 0 is empty"""
    S = vol.shape[0]
    out = vol.copy()
    for cx, cy, cz, r in np.asarray(items, np.int64).reshape(-1, 4):
        if r < 0:
            continue
        lo = [max(0, c - r) for c in (cx, cy, cz)]
        hi = [min(S, c + r + 1) for c in (cx, cy, cz)]
        if any(l >= h for l, h in zip(lo, hi)):
            continue
        x, y, z = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r] = value
    return out


def boxes(vol, items, value):
    S = vol.shape[0]
    out = vol.copy()
    for b in np.asarray(items, np.int64).reshape(-1, 6):
        hi = np.minimum(b[3:], S)
        out[b[0]:hi[0], b[1]:hi[1], b[2]:hi[2]] = value
    return out


def voxels(vol, items, value):
    S = vol.shape[0]
    out = vol.copy()
    p = np.asarray(items, np.int64).reshape(-1, 3)
    p = p[np.all(p < S, axis=1)]
    out[p[:, 0], p[:, 1], p[:, 2]] = value
    return out


def count_boxes(vol, items):
    S = vol.shape[0]
    out = []
    for b in np.asarray(items, np.int64).reshape(-1, 6):
        hi = np.minimum(b[3:], S)
        out.append(int(vol[b[0]:hi[0], b[1]:hi[1], b[2]:hi[2]].sum()) if np.all(b[:3] < hi) else 0)
    return np.array(out, np.uint64)


def get_voxels(vol, items):
    S = vol.shape[0]
    p = np.asarray(items, np.int64).reshape(-1, 3)
    ok = np.all(p < S, axis=1)
    out = np.zeros(len(p), np.uint8)
    out[ok] = vol[p[ok, 0], p[ok, 1], p[ok, 2]]
    return out


def window_of(first, capacity, T):
    """how many records of a list of T the window [first, first + capacity) holds"""
    return max(0, min(int(capacity), int(T) - int(first)))


@functools.lru_cache(maxsize=256)
def _records(model, shape, content, args):
    out = model(np.frombuffer(content, np.uint8).reshape(shape), *args)
    out.setflags(write=False)
    return out


def once(model, vol, *args):
    """model(vol, *args) of a family's model that lists records, computed once per content of the volume: a test runs a mirror
    of its own over the steps that the generator's mirror has just been through, and at 64^3 these lists are most of a
    program's time.  The records are shared: read only"""
    return _records(model, vol.shape, np.ascontiguousarray(vol, np.uint8).tobytes(), args)


def voxel_list(vol, a, which=None, neighbours=False):
    """the list a voxels / listToSecond step names, or that of another `which` over the same box"""
    box = None if a["box"] is None else tuple(int(q) for q in a["box"])
    return once(voxels_model.voxels_dense, vol, a.get("op", a.get("which")) if which is None else which, box, a["closed"], neighbours)


def stale_emit(records, offsets_of, S, first, capacity, n):
    """the first n records of the caller's buffer after an emit pass that found ANOTHER list's offsets in the block: a
    workgroup (256 occupancy words, key >> 13) starts where `offsets_of`'s voxels before it end, and returns early where those
    offsets show it nothing inside the window (vrc_list.h, list_window: the uniform return); what no workgroup writes keeps
    the guard"""
    groups = max(1, S ** 3 // 32 // 256)
    mine = surface_model.key_of(records[:, :3], S) >> 13
    start = np.concatenate([[0], np.cumsum(np.bincount(surface_model.key_of(offsets_of[:, :3], S) >> 13, minlength=groups))])
    out = np.full((n, records.shape[1]), GUARD, np.uint32)
    for g in range(groups):
        if start[g] == start[g + 1] or start[g + 1] <= first or start[g] >= first + capacity:
            continue
        rows = records[mine == g]
        at = start[g] + np.arange(len(rows)) - first
        ok = (at >= 0) & (at < n)
        out[at[ok]] = rows[ok]
    return out


def hits_of(cells, S, miss_every=5):
    """unit-voxel hit records whose vrc_hit_to_voxel voxel is `cells` (vrc.h:196-201: S-1 - floor((position - 1) S); the
    centre of the reflected cell is exact in float32 for S <= 64), normal (0, -2, 0): the neighbour is y + 1; every
    miss_every-th record is a miss"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    rec = np.zeros(len(cells), HIT_DTYPE)
    rec["hit"] = 1
    rec["hit"][::miss_every] = 0
    rec["position"] = (1.0 + (S - 1 - cells + 0.5) / S).astype(np.float32)
    rec["normal"][:, 1] = -2
    return rec


def hit_centres(rec, S, solid):
    """the centres of the brush: dig at the voxel, build at the neighbour where it lies inside"""
    ok = (rec["hit"] & 0xff) == 1
    cells = (S - 1 - np.floor((rec["position"][ok].astype(np.float64) - 1.0) * S)).astype(np.int64)
    if solid:
        cells = cells + [0, 1, 0]
        cells = cells[cells[:, 1] < S]
    return cells


def stroke_centres(rec, S, solid):
    """(centres (n, 3) int64, valid (n,) bool), one per RECORD as the stroke needs them: a miss, and a build without a
    neighbour, is no centre and breaks the stroke"""
    valid = ((rec["hit"] & 0xff) == 1) & np.all((rec["position"] >= 1) & (rec["position"] < 2), axis=1)        # vrc.h:217
    cells = (S - 1 - np.floor((rec["position"].astype(np.float64) - 1.0) * S)).astype(np.int64)
    if solid:
        cells = cells + [0, 1, 0]
        valid = valid & (cells[:, 1] < S)
    cells[~valid] = 0
    return cells, valid


def walk_cells(rng, S, n, reach=2):
    """n cells of a random walk with steps of at most `reach` a coordinate: the hits of a dragged crosshair"""
    return np.clip(rng.integers(0, S, 3) + np.cumsum(rng.integers(-reach, reach + 1, (n, 3)), axis=0), 0, S - 1)


def crossing_capsule(rng, S):
    """an item whose major axis crosses a multiple of 16 (at S > 16 inside the volume: the capsule has two pieces)"""
    m = 16 * int(rng.integers(1, S // 16)) if S > 16 else 0
    axis = int(rng.integers(0, 3))
    a, b = rng.integers(0, S, 3), rng.integers(0, S, 3)
    b = a + np.clip(b - a, -5, 5)
    a[axis], b[axis] = m - 6, m + 6
    return np.concatenate([a, b, [int(rng.integers(0, 3)), 0]]).astype(np.int32)


def clipped_raster_triangles(S):
    """a triangle wholly outside the volume in x and one with a coordinate over raster_model.LIMIT (dropped): nothing is selected"""
    U = raster_model.UNIT
    return np.array([[(S + 2) * U, U, U, (S + 5) * U, U, U, (S + 2) * U, 4 * U, U],
                     [U, U, U, raster_model.LIMIT + 1, U, U, U, 3 * U, 2 * U]], np.int32)


def rect_shape(rect, S):
    return (S, S) if rect is None else (max(0, int(rect[2]) - int(rect[0])), max(0, int(rect[3]) - int(rect[1])))


def box_mesh(lo, hi):
    """the 12 triangles of the box [lo, hi) in voxels, as surface_model.triangles winds them: a closed mesh"""
    q = []
    for d in range(6):
        a, s = d >> 1, d & 1
        u, v = (a + 1) % 3, (a + 2) % 3
        c = [[0, 0, 0] for _ in range(4)]
        for k, (du, dv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
            c[k][a] = hi[a] if s else lo[a]
            c[k][u] = hi[u] if du else lo[u]
            c[k][v] = hi[v] if dv else lo[v]
        order = (0, 1, 2, 0, 2, 3) if s else (0, 2, 1, 0, 3, 2)
        q += [c[i] for i in order]
    return (np.array(q, np.int64).reshape(12, 9) * voxelize_model.UNIT).astype(np.int32)


def clipped_triangles(S):
    """a degenerate triangle (n.z == 0) inside the volume and one wholly outside it in x: neither flips anything"""
    U = voxelize_model.UNIT
    return np.array([[U, U, U, U, U, 3 * U, U, U, 2 * U],
                     [(S + 2) * U, U, U, (S + 5) * U, U, U, (S + 2) * U, 4 * U, U]], np.int32)


# ---- the mirror --------------------------------------------------------------------------------------------------

class Mirror:
    """The dense occupancy of both volumes, the snapshots and the expected scratch.  apply(step) returns what the step's
    own query must observe (None for an edit) and sets .changed.  Arrays are replaced, never written in place, so that
    save() / restore() are shallow.  `fault`: one of FAULTS, the model of a library that has that hazard."""

    def __init__(self, depth, fault=None):
        self.depth, self.S, self.fault = depth, 1 << depth, fault
        S = self.S
        self.s = dict(v=np.zeros((S, S, S), np.uint8), w=np.zeros((S, S, S), np.uint8), clone=None, delta=None, stream=None, ids=None,
                      stage_v=0, blocks_v=frozenset(), stage_w=0, blocks_w=frozenset(),
                      marks_left=False, stage_tail=b"", rows_of=None, committed=None, before_edit=None, block_total=None)
        self.changed = False

    def save(self):
        return dict(self.s)

    def restore(self, saved):
        self.s = dict(saved)

    def scratch_bytes(self, which="v"):
        sizes = dict(d_marks=marks_bytes, d_surface=surface_bytes, d_rects=rects_bytes, d_pack=pack_bytes, d_flood=flood_bytes)
        return self.s["stage_" + which] + sum(sizes[b](self.depth) for b in self.s["blocks_" + which])

    def seen_download(self, which="v"):
        """what download() right behind the step shows"""
        if self.fault == "unordered" and which == "v" and self.s["before_edit"] is not None:
            return self.s["before_edit"]
        return self.s[which]

    def _stage(self, n_bytes, which="v"):
        self.s["stage_" + which] = max(self.s["stage_" + which], n_bytes)

    def _block(self, name, which="v"):
        self.s["blocks_" + which] = self.s["blocks_" + which] | {name}

    def _list_items(self, family, items, host):
        """the items a host-memory list edit reads: its own -- and, under the stage_tail fault, whatever whole items the
        block holds behind them"""
        raw = np.ascontiguousarray(items).tobytes()
        if host:
            tail = self.s["stage_tail"]
            if self.fault == "stage_tail" and len(tail) > len(raw):
                width = ITEM_BYTES[family]
                whole = (len(tail) - len(raw)) // width * width
                items = np.frombuffer(raw + tail[len(raw):len(raw) + whole], items.dtype).reshape(-1, items.shape[1])
            self.s["stage_tail"] = raw + tail[len(raw):]
        return items

    def _op(self, dst, bits, op):
        return cells_model.apply_op(dst, bits, op).astype(np.uint8)

    def apply(self, step):
        family, form, a = step
        s, S, depth = self.s, self.S, self.depth
        v0, w0 = s["v"], s["w"]
        host = form == "host"
        out = None
        s["before_edit"] = None
        if family in ("setVoxels", "fillBoxes", "fillSpheres"):
            items = self._list_items(family, a["items"], host)
            s["v"] = {"setVoxels": voxels, "fillBoxes": boxes, "fillSpheres": spheres}[family](v0, items, 1 if a["solid"] else 0)
            if host:
                self._stage(ITEM_BYTES[family] * len(a["items"]))
        elif family in ("fillCapsules", "rasterMesh"):
            items = self._list_items(family, a["items"], host)
            if family == "fillCapsules":
                s["v"] = stroke_model.fill_capsules(v0.copy(), items, 1 if a["solid"] else 0)
            else:
                s["v"] = raster_model.raster_mesh(S, items, a["op"], a["solid"], v0.copy())
            if host:
                self._stage(ITEM_BYTES[family] * len(a["items"]))
        elif family in AT_HITS:
            if family == "fillSpheresAtHits":
                centres = hit_centres(a["hits"], S, a["solid"])
                items = np.concatenate([centres, np.full((len(centres), 1), a["radius"], np.int64)], axis=1)
                s["v"] = spheres(v0, items, 1 if a["solid"] else 0)
            else:
                centres, valid = stroke_centres(a["hits"], S, a["solid"])
                if self.fault == "links" and not host and a.get("then") is not None:
                    # the host-memory call behind the stroke has rewritten the head of the block (its coordinates, 12 bytes
                    # an item) before k_stroke_links read it: n x (x, y, z, radius or -1) int32 as k_hits_to_centres left them
                    block = np.concatenate([centres, np.where(valid, a["radius"], -1)[:, None]], axis=1).astype(np.int32)
                    raw = bytearray(block.tobytes())
                    over = np.ascontiguousarray(a["then"][1], np.uint32).tobytes()[:len(raw)]
                    raw[:len(over)] = over
                    block = np.frombuffer(bytes(raw), np.int32).reshape(-1, 4).astype(np.int64)
                    centres, valid = block[:, :3], block[:, 3] >= 0
                items = stroke_model.stroke_items(centres, valid, a["radius"], a["max_gap"])
                s["v"] = stroke_model.fill_capsules(v0.copy(), items, 1 if a["solid"] else 0)
            self._stage((64 if host else 16) * len(a["hits"]))
            if host:
                s["stage_tail"] = np.ascontiguousarray(a["hits"]).tobytes() + s["stage_tail"][48 * len(a["hits"]):]
            if a.get("then") is not None:
                kind, items = a["then"]
                if kind == "setVoxels":
                    s["v"] = voxels(s["v"], self._list_items(kind, items, True), 1)
                    self._stage(12 * len(items))
                else:
                    out = get_voxels(s["v"] if self.fault != "unordered" else v0, items)
                    self._stage(13 * len(items))
        elif family == "xorMesh":
            field = s["v"].copy()
            if s["marks_left"]:                                   # a stale mark: the scan flips a column it should not
                field[1, 1, :max(1, S // 2)] ^= 1
                s["marks_left"] = False
            s["v"] = voxelize_model.xor_mesh(S, a["tris"], field)
            if self.fault == "marks" and a["kind"] != "box":
                s["marks_left"] = True
            self._block("d_marks")
            if host:
                self._stage(36 * len(a["tris"]))
                s["stage_tail"] = np.ascontiguousarray(a["tris"]).tobytes() + s["stage_tail"][36 * len(a["tris"]):]
        elif family == "copyRegion":
            lo, size, dst = a["src_lo"], a["size"], a["dst_lo"]
            view = tuple(slice(dst[k], dst[k] + size[k]) for k in range(3))
            bits = w0[tuple(slice(lo[k], lo[k] + size[k]) for k in range(3))]
            new = v0.copy()
            new[view] = self._op(new[view], bits, a["op"])
            s["v"] = new
        elif family == "stampAffine":
            s["v"] = stamp_model.stamp(v0, w0, a["m"], a["t"], a["lo"], a["hi"], a["op"])
        elif family == "fillRandom":
            s["v"] = cells_model.fill_random(v0, a["seed"], a["threshold"], a["box"], a["op"])
        elif family == "applyDelta":
            words = delta_model.apply(delta_model.words_of(v0), s["delta"])
            s["v"] = delta_model.dense_of(words, depth)
        elif family == "unpack":
            s["v"] = pack_model.unpack(s["stream"], depth)
            self._block("d_pack")
        elif family == "cellStepDst":
            s["v"] = cells_model.step(w0, a["birth"], a["survive"], a["neighbours"], a["outside"])[0]
        elif family == "cellStepSrc":
            s["w"] = cells_model.step(v0, a["birth"], a["survive"], a["neighbours"], a["outside"])[0]
        elif family == "fillColumns":
            s["v"] = columns_model.fill(v0, a["axis"], a["lo"], a["hi"], a["rect"], a["op"])        # no staging in v: OWN_BLOCK
        elif family == "selectColumnsDst":
            s["v"] = columns_model.select(v0, w0, a["direction"], a["lo"], a["hi"], a["of"], a["op"])
        elif family == "selectColumnsSrc":
            s["w"] = columns_model.select(w0, v0, a["direction"], a["lo"], a["hi"], a["of"], a["op"])
        elif family == "columnProfile":
            # a rect must be non-empty (vrc.h:1298): an empty one is refused and nothing moves
            out = "refused" if 0 in rect_shape(a["rect"], S) else columns_model.profile(v0, a["direction"], a["rect"])
        elif family == "floodRegion":
            s["v"] = flood_model.flood(w0, v0, a["connectivity"], a["through_empty"])
            self._block("d_flood")
            out = int(s["v"].sum())
        elif family == "floodMedium":
            s["w"] = flood_model.flood(v0, w0, a["connectivity"], a["through_empty"])
            self._block("d_flood", "w")
            out = int(s["w"].sum())
        elif family == "keepConnected":
            anchors = boxes(np.zeros_like(v0), a["anchors"], 1)
            s["v"] = flood_model.flood(v0, anchors, a["connectivity"])
            out = v0 & (1 - s["v"])                               # the debris
        elif family == "dilate":
            s["v"] = distance_model.dilate(v0, a["r"]).astype(np.uint8)
        elif family == "erode":
            s["v"] = distance_model.erode(v0, a["r"], a["open_border"]).astype(np.uint8)
        elif family == "select":
            s["v"] = self._op(v0, components_model.select(s["ids"], a["keep"]), a["op"])
        elif family == "place":
            s["v"] = fall_model.place(s["ids"], a["offsets"], v0, a["op"] == OR, a["keep"])
        elif family == "solidCount":
            out = int(v0.sum())
        elif family == "getVoxels":
            out = get_voxels(v0, a["items"])
            if host:
                self._stage(13 * len(a["items"]))
        elif family == "countBoxes":
            out = count_boxes(v0, a["items"])
            if host:
                self._stage(32 * len(a["items"]))
        elif family in ("surface", "rects"):
            # host form: the count, then the window.  Device forms: (counts, window, total); with order "extract_first" the
            # extraction is still on its stream when the synchronous count of the OTHER `closed` rewrites the shared block
            # (vrc.h:271-272: the extraction is recorded as the last asynchronous edit, so the count waits for it)
            seen = v0
            if family == "rects":
                seen = s["rows_of"] if self.fault == "rows" and s["rows_of"] is not None else v0
                s["rows_of"] = seen
            model = (lambda closed: once(surface_model.faces, seen, closed)) if family == "surface" else (lambda closed: once(rect_model.rects, seen, closed))
            tally = surface_model.direction_counts if family == "surface" else rect_model.direction_counts
            records = model(a["closed"])
            first_extract = not host and a.get("order") == "extract_first"
            counted = model(not a["closed"]) if first_extract else records
            if first_extract and self.fault == "unordered":
                records = counted                                 # the extraction reads the offsets the count left
            window = records[a["first"]:a["first"] + a["capacity"]]
            counts = tally(counted)
            if family == "surface":
                s["block_total"] = len(records)
                if not host and a.get("order") == "voxels_behind":
                    # the extraction is still on its stream when a synchronous voxelCount rewrites the offsets block, the total
                    # behind the last slot included (vrc.h:444-447, 454-455: the count waits for the extraction)
                    behind = voxel_list(v0, a["behind"])
                    counts = s["block_total"] = len(behind)
                    if self.fault == "unordered":
                        window = stale_emit(records, behind, S, a["first"], a["capacity"], len(window))
            out = (counts, window) if host else (counts, window, len(records))
            self._block("d_" + family)
            if host and len(window):
                self._stage(16 * len(window))
        elif family == "voxels":
            # host form: voxelCount, then the window.  Device forms: (counts, window, total) with the records in a buffer of the
            # test's own; `counts` is the step's own voxelCount issued first ("count_first"), or, issued right behind the
            # extraction still on its stream, the voxelCount of another `which` ("extract_first") or the six totals of
            # surfaceCount ("surface_behind"), which keeps its direction totals in the same block
            records = voxel_list(v0, a, neighbours=a["neighbours"])
            T = len(records)
            n = window_of(a["first"], a["capacity"], T)
            window = records[a["first"]:a["first"] + n]
            total_left = T
            if host:
                if self.fault == "totals" and s["block_total"] is not None:
                    # the window is sized by the total the block held on entry; what the pass does not emit stays zero
                    n = window_of(a["first"], a["capacity"], s["block_total"])
                    window = np.concatenate([window, np.zeros((n, window.shape[1]), np.uint32)])[:n]
                out = (T, window)
                if n:
                    self._stage((16 if a["neighbours"] else 12) * min(n, 1 << 20))
            elif a["order"] == "extract_first":
                other = voxel_list(v0, a, (a["op"] + a["shift"]) % 3)
                if self.fault == "unordered":
                    window = stale_emit(records, other, S, a["first"], a["capacity"], n)
                out = (len(other), window, T)
                total_left = len(other)
            elif a["order"] == "surface_behind":
                # surfaceCount writes the six direction totals alone, behind the slot of the total (vrc_surface.hip, surface_direction_slots and surface_count_run):
                # slots that no pass of the lists reads, so even unordered it leaves the extraction what it was
                out = (surface_model.direction_counts(once(surface_model.faces, v0, a["closed"])), window, T)
            else:
                out = (T, window, T)
            s["block_total"] = total_left
            self._block("d_surface")
        elif family == "listToSecond":
            items = voxel_list(v0, a)
            assert self.fault is not None or a["n"] == len(items)     # the length the step hands to setVoxelsDevice is the mirror's
            s["w"] = voxels(w0, items, 1 if a["solid"] else 0)
            s["block_total"] = len(items)
            self._block("d_surface")
        elif family == "pack":
            s["stream"] = pack_model.pack(v0, depth)
            out = s["stream"]
            self._block("d_pack")
        elif family == "diff":
            s["delta"], stats = delta_model.diff(delta_model.words_of(s["clone"]), delta_model.words_of(v0), depth)
            out = (s["delta"], delta_model.stats_tuple(stats))
        elif family == "components":
            out = components_model.label(v0, a["connectivity"])[1]
        elif family == "distanceAt":
            D = distance_model.field(v0, a["to_empty"], a["outside"])
            p = np.asarray(a["items"], np.int64)
            out = D[p[:, 0], p[:, 1], p[:, 2]].astype(np.uint32)
        elif family == "commit":
            out = v0 if self.fault != "commit" or s["committed"] is None else (v0 | s["committed"])
            s["committed"] = v0
        elif family in REFUSALS:
            out = "refused"
        elif family == "cloneSecond":
            s["w"], s["stage_w"], s["blocks_w"] = v0, 0, frozenset()
        elif family == "recreateSecond":
            s["w"] = cells_model.fill_random(np.zeros_like(v0), a["seed"], a["threshold"])
            s["stage_w"], s["blocks_w"] = 0, frozenset()
        elif family == "snapshotLabels":
            s["ids"], records = components_model.label(v0, a["connectivity"])
            out = len(records)
        elif family == "snapshotClone":
            s["clone"] = v0
        else:
            raise ValueError(family)
        self.changed = not (np.array_equal(s["v"], v0) and np.array_equal(s["w"], w0))
        if family in EDITS and not host and family not in EDITS_OF_W:
            s["before_edit"] = v0
        return out


@functools.lru_cache(maxsize=None)
def empty_stream_bytes(depth):
    S = 1 << depth
    return len(pack_model.pack(np.zeros((S, S, S), np.uint8), depth))


def is_empty(out):
    """a query's result that shows nothing: None, zero, or all parts empty / all zero"""
    if out is None:
        return True
    if isinstance(out, (tuple, list)):
        return all(is_empty(o) for o in out)
    if isinstance(out, (bytes, bytearray)):
        return len(out) == empty_stream_bytes(pack_model.header_of(out)[2])       # as long as an empty volume's stream
    if isinstance(out, np.ndarray):
        return out.size == 0 or (out.dtype.names is None and not out.any())
    return out == 0


# ---- the generator -----------------------------------------------------------------------------------------------

def _box(rng, S, least=1):
    lo = rng.integers(0, S - least + 1, 3)
    size = np.array([rng.integers(least, S - l + 1) for l in lo])
    size = np.minimum(size, max(least, S // 2 + 1))
    return [int(q) for q in lo], [int(q) for q in size]


def _rect(rng, S):
    """a non-empty rect of columns (u_lo, v_lo, u_hi, v_hi) inside the face"""
    u_lo, v_lo = int(rng.integers(0, S)), int(rng.integers(0, S))
    return [u_lo, v_lo, int(rng.integers(u_lo + 1, S + 1)), int(rng.integers(v_lo + 1, S + 1))]


BOX_KINDS = ("whole", "cut", "beyond", "empty")


def _voxel_box(rng, S, kind):
    """the box of a voxel list: the whole volume (None or spelled out); one that cuts occupancy words on all three axes (odd
    bounds in x and y, z bounds that are no multiples of 8); one reaching beyond the volume; an empty one"""
    if kind == "whole":
        return None if rng.random() < 0.5 else [0, 0, 0, S, S, S]
    if kind == "cut":
        lo = [1 + 2 * int(rng.integers(0, S // 4)), 1 + 2 * int(rng.integers(0, S // 4)), int(rng.integers(1, S // 2))]
        hi = [S // 2 + 1 + 2 * int(rng.integers(0, S // 4)), S // 2 + 1 + 2 * int(rng.integers(0, S // 4)), int(rng.integers(S // 2 + 1, S))]
        lo[2] += lo[2] % 8 == 0
        hi[2] -= hi[2] % 8 == 0
        return lo + hi
    lo = [int(q) for q in rng.integers(0, S // 2, 3)]
    if kind == "beyond":
        return lo + [int(rng.choice([S + 1, S + 100, 0xFFFFFFFF])) for _ in range(3)]
    hi = [q + 1 + int(rng.integers(0, S // 2)) for q in lo]
    axis = int(rng.integers(0, 3))
    if rng.random() < 0.5:
        hi[axis] = lo[axis]                                                   # nothing between lo and hi
    else:
        lo[axis], hi[axis] = S + 2, S + 5                                     # wholly outside
    return lo + hi


def _arguments(rng, family, form, m, op=None):
    """the arguments of one step on the mirror's present state, or None where the family cannot run yet"""
    S, depth, s = m.S, m.depth, m.s
    a = {}
    if family in ("setVoxels", "fillBoxes", "fillSpheres", "fillSpheresAtHits", "fillCapsules", "strokeAtHits", "rasterMesh"):
        a["solid"] = bool(rng.integers(0, 2))
    if family in ("setVoxels", "getVoxels"):
        n = int(rng.integers(1, 40)) if rng.random() < 0.7 else int(rng.integers(60, 200))
        a["items"] = rng.integers(0, S + 1, (n, 3)).astype(np.uint32)
        if family == "getVoxels" and s["v"].any():
            solid = np.argwhere(s["v"])
            a["items"][::2] = solid[rng.integers(0, len(solid), len(a["items"][::2]))]
    elif family in ("fillBoxes", "countBoxes"):
        n = int(rng.integers(1, 4)) if rng.random() < 0.7 else int(rng.integers(20, 60))
        rows = []
        for _ in range(n):
            lo, size = _box(rng, S)
            size = [min(q, max(1, S // 4)) for q in size] if family == "fillBoxes" else size
            rows.append(lo + [l + q for l, q in zip(lo, size)])
        a["items"] = np.array(rows, np.uint32)
    elif family == "fillSpheres":
        n = int(rng.integers(1, 4)) if rng.random() < 0.7 else int(rng.integers(30, 80))
        a["items"] = np.concatenate([rng.integers(-1, S + 1, (n, 3)), rng.integers(0, max(2, S // 8) + 1, (n, 1))], axis=1).astype(np.int32)
    elif family == "fillSpheresAtHits":
        n = int(rng.integers(3, 30))
        a["hits"] = hits_of(rng.integers(0, S, (n, 3)), S)
        a["radius"] = int(rng.integers(0, max(1, S // 16) + 1))
        a["then"] = None
        if form in ("devA", "devB") and rng.random() < 0.7:
            items = rng.integers(0, S, (int(rng.integers(1, 5)), 3)).astype(np.uint32)
            a["then"] = ("setVoxels" if rng.random() < 0.5 else "getVoxels", items)
    elif family == "fillCapsules":
        # degenerate, axis-aligned, exact diagonals, ends far outside, r = -1 and dropped items, as the brush's own test draws
        # them, and one capsule of more than one piece
        n = int(rng.integers(1, 6)) if rng.random() < 0.7 else int(rng.integers(20, 50))
        a["items"] = np.concatenate([stroke_model.mixed_items(rng, S, n), crossing_capsule(rng, S)[None, :]])
    elif family == "strokeAtHits":
        n = int(rng.integers(3, 30))
        a["hits"] = hits_of(walk_cells(rng, S, n), S)
        a["radius"], a["max_gap"] = int(rng.choice([0, 1, 3])), int(rng.choice([0, 2]))
        a["then"] = None
        if form in ("devA", "devB") and rng.random() < 0.7:
            items = rng.integers(0, S, (int(rng.integers(1, 5)), 3)).astype(np.uint32)
            a["then"] = ("setVoxels" if rng.random() < 0.5 else "getVoxels", items)
    elif family == "rasterMesh":
        a["op"] = int(rng.integers(0, 2))                                     # the mode
        a["kind"] = ("small", "small", "small", "mixed", "span", "clipped")[int(rng.integers(0, 6))]
        n = int(rng.integers(1, 6)) if rng.random() < 0.7 else int(rng.integers(20, 50))
        small = raster_model.small_triangles(rng, S, n).astype(np.int32)
        a["items"] = {"small": small, "mixed": np.concatenate([clipped_raster_triangles(S), small]), "clipped": clipped_raster_triangles(S),
                      "span": raster_model.corner_triangle(S).astype(np.int32)}[a["kind"]]
    elif family == "columnProfile":
        a["direction"] = int(rng.integers(0, 6))
        pick = rng.random()
        a["rect"] = None if pick < 0.4 else _rect(rng, S)
        if pick > 0.92:
            a["rect"][2] = a["rect"][0]                                       # empty: refused
    elif family == "fillColumns":
        a["axis"], a["rect"], a["op"] = int(rng.integers(0, 3)), _rect(rng, S), int(rng.integers(0, 3))
        shape = rect_shape(a["rect"], S)
        # host memory: one map or two; device memory: constants alone, or maps there
        maps = int(rng.integers(1, 3)) if form == "host" else int(rng.integers(0, 3))
        which = (0, 1) if maps == 2 else (int(rng.integers(0, 2)),) if maps == 1 else ()
        lo, hi = int(rng.integers(-2, S // 2 + 1)), int(rng.integers(S // 2, S + 3))
        bounds = [rng.integers(-3, S + 4, shape).astype(np.int32) if k in which else c for k, c in enumerate((lo, hi))]
        a["lo"], a["hi"], a["maps"] = bounds[0], bounds[1], maps
    elif family in ("selectColumnsDst", "selectColumnsSrc"):
        a["direction"], a["of"], a["op"] = int(rng.integers(0, 6)), int(rng.choice([columns_model.SOLID, columns_model.EMPTY, columns_model.BOTH])), int(rng.integers(0, 3))
        a["lo"] = int(rng.integers(0, max(2, S // 4)))
        a["hi"] = (a["lo"], a["lo"] + 1, a["lo"] + int(rng.integers(1, S)), S + 1 + int(rng.integers(1, 9)))[int(rng.integers(0, 4))]
    elif family == "xorMesh":
        a["kind"] = ("box", "box", "mixed", "clipped")[int(rng.integers(0, 4))]
        lo, size = _box(rng, S)
        mesh = box_mesh(lo, [l + q for l, q in zip(lo, size)])
        a["tris"] = {"box": mesh, "mixed": np.concatenate([clipped_triangles(S), mesh]), "clipped": clipped_triangles(S)}[a["kind"]]
    elif family == "copyRegion":
        a["src_lo"], a["size"] = _box(rng, S)
        a["dst_lo"] = [int(rng.integers(0, S - q + 1)) for q in a["size"]]
        a["op"] = int(rng.integers(0, 3))
    elif family == "stampAffine":
        perms = stamp_model.all_signed_permutations()
        perm, flip = perms[int(rng.integers(0, len(perms)))]
        a["m"], a["t"] = stamp_model.signed_permutation(perm, flip, S)
        lo, size = _box(rng, S)
        a["lo"], a["hi"], a["op"] = lo, [l + q for l, q in zip(lo, size)], int(rng.integers(0, 3))
    elif family == "fillRandom":
        lo, size = _box(rng, S)
        a["seed"], a["threshold"] = int(rng.integers(0, 1 << 32)), cells_model.threshold_of(float(rng.choice([0.1, 0.3, 0.6])))
        a["box"], a["op"] = lo + [l + q for l, q in zip(lo, size)], int(rng.integers(0, 3))
    elif family == "applyDelta":
        if s["delta"] is None:
            return None
    elif family == "unpack":
        if s["stream"] is None:
            return None
        a["device"] = form != "host"
    elif family in ("cellStepDst", "cellStepSrc"):
        a["neighbours"] = int(rng.choice([6, 26]))
        top = a["neighbours"]
        a["birth"] = cells_model.SMOOTH_BIRTH if top == 26 else sum(1 << c for c in range(3, 7))
        a["survive"] = cells_model.SMOOTH_SURVIVE if top == 26 else sum(1 << c for c in range(2, 7))
        a["outside"] = int(rng.integers(0, 2))
    elif family in ("floodRegion", "floodMedium"):
        a["connectivity"], a["through_empty"] = int(rng.choice([6, 26])), bool(rng.integers(0, 2))
    elif family == "keepConnected":
        lo, size = _box(rng, S, max(1, S // 4))
        a["anchors"], a["connectivity"] = np.array([lo + [l + q for l, q in zip(lo, size)]], np.uint32), int(rng.choice([6, 26]))
    elif family in ("dilate", "erode"):
        a["r"] = int(rng.integers(1, 3))
        a["open_border"] = bool(rng.integers(0, 2))
    elif family in ("select", "place"):
        if s["ids"] is None:
            return None
        count = int(s["ids"][s["ids"] != components_model.NO_COMPONENT].max()) + 1 if (s["ids"] != components_model.NO_COMPONENT).any() else 0
        if count == 0:
            return None
        a["keep"] = (rng.random(count) < 0.6).astype(np.uint8)
        a["keep"][int(rng.integers(0, count))] = 1
        a["op"] = int(rng.integers(0, 3)) if family == "select" else int(rng.choice([OR, ANDNOT]))
        if family == "place":
            a["offsets"] = rng.integers(-2, 3, (count, 3)).astype(np.int32)
    elif family in ("surface", "rects"):
        a["closed"], a["first"], a["capacity"] = bool(rng.integers(0, 2)), int(rng.integers(0, 8)), int(rng.integers(1, 400))
        a["order"] = ("count_first", "extract_first")[int(rng.integers(0, 2))]
        if family == "surface" and rng.random() < 1 / 3:
            # the voxelCount that rewrites the shared block right behind the extraction
            a["order"] = "voxels_behind"
            a["behind"] = dict(op=int(rng.integers(0, 3)), box=_voxel_box(rng, S, ("whole", "cut", "beyond")[int(rng.integers(0, 3))]), closed=bool(rng.integers(0, 2)))
    elif family in ("voxels", "listToSecond"):
        a["kind"] = ("whole", "whole", "cut", "cut", "beyond", "empty")[int(rng.integers(0, 6))]
        a["box"], a["closed"] = _voxel_box(rng, S, a["kind"]), bool(rng.integers(0, 2))
        if family == "voxels":
            a["op"], a["neighbours"] = int(rng.integers(0, 3)), bool(rng.integers(0, 2))
            a["first"], a["capacity"] = int(rng.integers(0, 8)), int(rng.integers(1, 400))
            # device forms: the output 4- but not 8-byte aligned (x y z alone); what runs around the extraction; `shift`: which
            # other `which` the count behind the extraction takes
            a["skew"] = 0 if a["neighbours"] else 4 * int(rng.integers(0, 2))
            a["order"] = ("count_first", "extract_first", "surface_behind")[int(rng.integers(0, 3))]
            a["shift"] = int(rng.integers(1, 3))
        else:
            a["which"], a["solid"] = int(rng.integers(0, 3)), bool(rng.integers(0, 2))
            a["n"] = len(voxel_list(s["v"], a))                               # the list's length, which the caller of setVoxelsDevice must know
    elif family in ("components", "snapshotLabels"):
        a["connectivity"] = int(rng.choice([6, 26]))
    elif family == "distanceAt":
        a["to_empty"], a["outside"] = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        a["items"] = rng.integers(0, S, (int(rng.integers(1, 30)), 3)).astype(np.uint32)
    elif family == "diff":
        if s["clone"] is None:
            return None
    elif family == "recreateSecond":
        a["seed"], a["threshold"] = int(rng.integers(0, 1 << 32)), cells_model.threshold_of(0.4)
    elif family in ("refusePack", "refuseUnpack"):
        if s["stream"] is None or "d_pack" not in s["blocks_v"]:
            return None
        if family == "refuseUnpack":
            made = pack_model.corruptions(s["stream"])
            rule, variant, data, _ = made[int(rng.integers(0, len(made)))]
            a["rule"], a["data"] = rule, bytes(data)
    elif family == "refuseDelta":
        a["records"] = np.array([[5, 1], [3, 2]], np.uint32)                  # word 3 behind word 5: not ascending
    if op is not None and "op" in a:
        a["op"] = op
    return a


_FORMS_OF = {
    **{f: FORMS for f in LIST_EDITS + ("getVoxels", "countBoxes", "surface", "rects", "columnProfile", "fillColumns", "voxels")},
    **{f: FORMS[1:] for f in STREAM_EDITS + ("listToSecond",)},
    "unpack": ("host", "dev0"), "pack": ("host", "dev0"), "select": FORMS,
}


OPS_OF = {"copyRegion": (REPLACE, OR, ANDNOT), "stampAffine": (REPLACE, OR, ANDNOT), "fillRandom": (REPLACE, OR, ANDNOT),
          "select": (REPLACE, OR, ANDNOT), "place": (OR, ANDNOT), "rasterMesh": (TOUCHED, THIN), "fillColumns": (REPLACE, OR, ANDNOT),
          "selectColumnsDst": (REPLACE, OR, ANDNOT), "selectColumnsSrc": (REPLACE, OR, ANDNOT),
          "voxels": (voxels_model.ALL, voxels_model.SURFACE, voxels_model.INTERIOR)}
ALL_FORMS = LIST_EDITS + ("getVoxels", "countBoxes", "surface", "rects", "columnProfile", "fillColumns", "voxels")
# (family, op, form) for every family, every op of the families that take one and every form of the list calls (None: any
# form): the tour that every depth's programs run in full
TOUR = tuple((family, op, form) for family in FAMILIES for op in OPS_OF.get(family, (None,)) for form in (FORMS if family in ALL_FORMS else (None,)))


def _circuit(nodes):
    """a closed walk that takes every ordered pair of `nodes` (a node with itself included) exactly once: Hierholzer on
    the complete directed graph with loops, edges taken in the order of `nodes`"""
    left = {a: list(nodes) for a in nodes}
    stack, walk = [nodes[0]], []
    while stack:
        if left[stack[-1]]:
            stack.append(left[stack[-1]].pop(0))
        else:
            walk.append(stack.pop())
    return tuple(reversed(walk))


STAGE_WALK = _circuit(BLOCKS["d_stage"])          # 169 pairs
PACK_WALK = _circuit(BLOCKS["d_pack"])            # 16 pairs
SURFACE_WALK = _circuit(BLOCKS["d_surface"])      # 9 pairs


def _share(walk, index, of):
    """the index-th of `of` stretches of a walk, overlapping by one node so that no pair is lost"""
    edges = len(walk) - 1
    per = -(-edges // of)
    return walk[index * per:min(index * per + per, edges) + 1] if index * per < edges else ()


PROLOGUE = (
    # what the coverage conditions name, once each in every program, before the seeded part
    ("fillRandom", "dev0", dict(seed=7, threshold=cells_model.threshold_of(0.5), box=None, op=OR)),
    ("cellStepSrc", "dev0", dict(neighbours=26, birth=cells_model.SMOOTH_BIRTH, survive=cells_model.SMOOTH_SURVIVE, outside=1)),
    ("snapshotClone", "host", {}),
    ("snapshotLabels", "host", dict(connectivity=6)),
    ("commit", "host", {}),
    ("refuseVoxels", "host", {}),                      # before any surface or voxel call: a refusal reserves no offsets block
    ("refuseVoxelsAligned", "host", {}),
    ("rects", "host", dict(closed=True, first=0, capacity=50)),
    ("surface", "host", dict(closed=True, first=0, capacity=50)),
)


class _Writer:
    """a program being written: the steps so far and the mirror after them"""

    def __init__(self, seed, depth):
        self.rng, self.m, self.out, self.seen = np.random.default_rng(seed), Mirror(depth), [], []

    def emit(self, step):
        seen = self.m.apply(step)
        self.record(step, seen)
        return seen

    def record(self, step, own):
        m = self.m
        self.out.append(step)
        self.seen.append((own, m.seen_download("v"), m.s["w"], m.scratch_bytes("v"), m.scratch_bytes("w"), m.changed, m.s["stage_v"]))

    def solid(self, n):
        """n solid voxels of v (fewer where it holds fewer; one is set first where it holds none)"""
        if not self.m.s["v"].any():
            self.emit(("setVoxels", "host", dict(items=np.array([[1, 1, 1]], np.uint32), solid=True)))
        at = np.argwhere(self.m.s["v"])
        return at[self.rng.permutation(len(at))[:n]].astype(np.uint32)

    def ready(self, family, pad=True):
        """what the family needs before it can run: a delta, a stream, a labelling with pieces"""
        s = self.m.s
        if pad and family in EDITS and not s["v"].any():                  # an emptied volume shows nothing of a clearing op
            self.emit(("fillRandom", "dev0", dict(seed=int(self.rng.integers(0, 1 << 32)), threshold=cells_model.threshold_of(0.4), box=None, op=OR)))
        if pad and family in ("copyRegion", "stampAffine", "cellStepDst", "floodRegion", "selectColumnsDst") and s["w"].mean() < 1 / 16:
            # (nearly) empty, as a narrow selectColumnsSrc band leaves it: nothing to copy, stamp or select from
            self.emit(("recreateSecond", "host", dict(seed=int(self.rng.integers(0, 1 << 32)), threshold=cells_model.threshold_of(0.4))))
        if family in ("select", "place") and (s["ids"] is None or not (s["ids"] != components_model.NO_COMPONENT).any()):
            self.solid(1)
            self.emit(("snapshotLabels", "host", dict(connectivity=6)))
        if family == "diff" and s["clone"] is None:
            self.emit(("snapshotClone", "host", {}))
        if family == "applyDelta" and s["delta"] is None:
            self.ready("diff")
            self.emit(("diff", "host", {}))
        if family in ("unpack", "refusePack", "refuseUnpack") and (s["stream"] is None or "d_pack" not in s["blocks_v"]):
            self.emit(("pack", "host", {}))
        if pad and family == "unpack" and np.array_equal(pack_model.unpack(self.m.s["stream"], self.m.depth), self.m.s["v"]):
            self.one("fillBoxes")                                 # so that the stream holds something else than the volume

    def one(self, family, form=None, op=None, tries=8, pad=True):
        """one step of the family with seeded arguments; an edit that changes nothing or a query that shows nothing is drawn
        again, up to `tries` times"""
        self.ready(family, pad)           # pad=False: nothing but the prerequisites, so that a walk's pairs stay adjacent
        for attempt in range(tries):
            forms = _FORMS_OF.get(family, ("host",))
            chosen = form if form is not None else forms[int(self.rng.integers(0, len(forms)))]
            step = (family, chosen, _arguments(self.rng, family, chosen, self.m, op))
            saved = self.m.save()
            seen = self.m.apply(step)
            idle = (family in EDITS and not self.m.changed) or (family in QUERIES and is_empty(seen))
            if idle and attempt < tries - 1:
                self.m.restore(saved)
                continue
            self.record(step, seen)
            return


def _scripted(w):
    """the step sequences that the coverage conditions and the fault switches need, on the mirror's state after PROLOGUE"""
    S = w.m.S
    U = S // 2
    many = np.array([[x, y, z] for x in range(min(S, 6)) for y in range(min(S, 6)) for z in range(2)], np.uint32)
    few = np.array([[S - 1, S - 1, S - 1]], np.uint32)
    for step in (
        ("fillBoxes", "host", dict(items=np.array([[0, 0, 0, U, S, S]], np.uint32), solid=False)),        # lowers the solid count
        ("commit", "host", {}),
        ("commit", "host", {}),
        ("rects", "host", dict(closed=True, first=0, capacity=50)),
        ("surface", "host", dict(closed=True, first=0, capacity=50)),
        ("setVoxels", "host", dict(items=many, solid=True)),                                              # larger list ...
        ("setVoxels", "host", dict(items=few, solid=False)),                                              # ... then smaller
        ("fillSpheresAtHits", "devA", dict(hits=hits_of(many[:7] + [0, 1, 0], S), radius=0, solid=False, then=None)),
        ("setVoxels", "host", dict(items=few, solid=True)),
        ("refuseMesh", "host", {}),
        ("xorMesh", "host", dict(kind="box", tris=box_mesh([0, 0, 0], [1, 1, 1]))),
        ("xorMesh", "devA", dict(kind="clipped", tris=clipped_triangles(S))),
        ("xorMesh", "host", dict(kind="box", tris=box_mesh([S - 1, 0, 0], [S, 1, 1]))),
        ("recreateSecond", "host", dict(seed=3, threshold=cells_model.threshold_of(0.4))),
        ("floodMedium", "host", dict(connectivity=26, through_empty=False)),                              # an edit of w ...
        ("floodRegion", "host", dict(connectivity=6, through_empty=False)),                               # ... then w as the medium of v
        ("floodRegion", "host", dict(connectivity=26, through_empty=False)),
        ("solidCount", "host", {}),
        ("solidCount", "host", {}),
        ("floodRegion", "host", dict(connectivity=26, through_empty=False)),
    ):
        w.emit(step)
    # inside ONE step, with no download between: a brush on a stream of the test's own, its centres in flight in the staging
    # block, and right behind it a host-memory list edit -- then a host-memory query of exactly the voxels the brush digs,
    # which sees them solid unless it waits for the brush
    w.emit(("fillSpheresAtHits", "devA", dict(hits=hits_of(w.solid(9), S, miss_every=10), radius=0, solid=False, then=("setVoxels", few))))
    dug = w.solid(9)
    w.emit(("fillSpheresAtHits", "devB", dict(hits=hits_of(dug, S, miss_every=10), radius=0, solid=False, then=("getVoxels", dug[1:]))))
    # inside ONE step: an extraction still on its stream while the synchronous count of the other `closed` uses the block;
    # the corner box makes the two meshes differ in the first records
    w.emit(("fillBoxes", "dev0", dict(items=np.array([[0, 0, 0, 2, 2, 2]], np.uint32), solid=True)))
    w.emit(("surface", "devA", dict(closed=True, first=0, capacity=60, order="extract_first")))
    w.emit(("surface", "devB", dict(closed=False, first=2, capacity=60, order="count_first")))
    w.emit(("rects", "devB", dict(closed=True, first=0, capacity=60, order="extract_first")))
    w.emit(("rects", "devA", dict(closed=False, first=2, capacity=60, order="count_first")))
    # the capsule brush, the surface voxelisation and the column calls on the same long-lived pair
    Q = min(S, 5)
    capsules = np.array([[i % S, 0, 0, i % S, S - 1, i % Q, i % 2, 0] for i in range(10)], np.int32)
    U64 = raster_model.UNIT
    sheet = np.array([[0, 0, U64 + 7, S * U64, 0, U64 + 7, 0, S * U64, U64 + 7]], np.int32)           # half of the plane z = 1 + 7/64
    one = np.full((3, Q), S // 2, np.int32)
    for step in (
        ("fillCapsules", "host", dict(items=capsules, solid=True)),                                       # 320 bytes of staging ...
        ("columnProfile", "host", dict(direction=5, rect=[0, 0, 3, Q])),                                  # ... then 16 x 3 x Q of records out
        ("fillColumns", "host", dict(axis=1, rect=[0, 0, 3, Q], op=REPLACE, lo=0, hi=one, maps=1)),       # one map ...
        ("fillColumns", "host", dict(axis=1, rect=[0, 0, 3, Q], op=OR, lo=one - 1, hi=one + 1, maps=2)),  # ... then two
        ("refuseRaster", "host", {}),
        ("rasterMesh", "host", dict(kind="small", op=TOUCHED, items=sheet, solid=False)),
        ("rasterMesh", "devB", dict(kind="clipped", op=THIN, items=clipped_raster_triangles(S), solid=True)),
        ("rasterMesh", "host", dict(kind="small", op=THIN, items=sheet, solid=True)),
        ("refuseStroke", "host", {}),
        ("strokeAtHits", "devA", dict(hits=hits_of(many[:6] + [0, 1, 0], S), radius=1, max_gap=0, solid=False, then=None)),
        ("fillCapsules", "host", dict(items=capsules[:2], solid=True)),                                   # a host staging call behind the stroke
    ):
        w.emit(step)
    # inside ONE step: the stroke's kernel reads centre i and i + 1 in the staging block while, right behind it, a host-memory
    # list edit comes to rewrite the block's head -- with four far corners, which as centres would join up along the edges --
    # and a host-memory query of exactly the voxels the stroke digs
    corners = np.array([[0, 0, 0], [S - 1, S - 1, 0], [0, S - 1, S - 1], [S - 1, 0, S - 1]], np.uint32)
    w.emit(("fillBoxes", "host", dict(items=np.array([[0, 0, 0, S, S, 1], [0, S - 1, 0, S, S, S]], np.uint32), solid=False)))
    w.emit(("strokeAtHits", "devB", dict(hits=hits_of(w.solid(9), S, miss_every=10), radius=0, max_gap=0, solid=True, then=("setVoxels", corners))))
    dug = w.solid(9)
    w.emit(("strokeAtHits", "devA", dict(hits=hits_of(dug, S, miss_every=10), radius=0, max_gap=0, solid=False, then=("getVoxels", dug[1:]))))
    _scripted_lists(w, many)


def _scripted_lists(w, many):
    """the voxel lists: their host windows in the staging block, and their passes in the offsets block of the surface calls"""
    m, S = w.m, w.m.S
    ALL, SURFACE, INTERIOR = voxels_model.ALL, voxels_model.SURFACE, voxels_model.INTERIOR
    cut = [1, 1, 1, S - 1, S - 1, S // 2 + 1]                                 # odd in x and y, no multiple of 8 in z
    beyond = [0, 0, 0, S + 1, 0xFFFFFFFF, S + 100]

    def lists(form, op, box, kind, neighbours, first, capacity, closed=True, **device):
        return ("voxels", form, dict(op=op, box=box, kind=kind, closed=closed, neighbours=neighbours, first=first, capacity=capacity, **device))

    # a slab four voxels thick: at least 64 voxels, some of them interior, at every depth
    w.emit(("fillBoxes", "dev0", dict(items=np.array([[0, 0, 0, S, S, min(S, 4)]], np.uint32), solid=True)))
    # a host window directly behind a larger host list edit; one that grows the staging block to exactly its own size; an empty
    # one, behind the end of a list that is not empty, which leaves the block alone
    w.emit(("setVoxels", "host", dict(items=many, solid=True)))
    w.emit(lists("host", SURFACE, None, "whole", False, 1, 3))
    grow = m.s["stage_v"] // 16 + 1
    assert len(voxel_list(m.s["v"], dict(op=ALL, box=None, closed=False))) >= grow
    w.emit(lists("host", ALL, [0, 0, 0, S, S, S], "whole", True, 0, grow, closed=False))
    assert m.s["stage_v"] == 16 * grow
    assert w.emit(lists("host", INTERIOR, None, "whole", True, 8 ** m.depth, 10))[0] > 0
    # inside ONE step: a voxel extraction still on its stream while a synchronous count -- of another `which`, then of the
    # surface calls, which keep their totals in the same block -- comes on the NULL stream; and a surface extraction with a
    # voxelCount behind it.  Each count differs from the total of the extraction it follows, and the windows begin where the
    # count's list ends: by the count's offsets no workgroup has a record in them.
    inner = len(voxel_list(m.s["v"], dict(op=INTERIOR, box=beyond, closed=True)))
    own = w.emit(lists("devA", ALL, beyond, "beyond", False, inner, 60, skew=4, order="extract_first", shift=2))
    assert own[0] == inner < own[2]
    w.emit(lists("devB", SURFACE, [2, 2, 2, 2, 3, 3], "empty", True, 0, 5, skew=0, order="surface_behind", shift=1))
    own = w.emit(lists("devB", INTERIOR, cut, "cut", False, 0, 60, skew=0, order="surface_behind", shift=1))
    assert own[2] > 0 and int(own[0].sum()) != own[2]
    own = w.emit(("surface", "devA", dict(closed=True, first=8, capacity=60, order="voxels_behind", behind=dict(op=ALL, box=[1, 1, 1, 3, 3, 3], closed=True))))
    assert 0 < own[0] <= 8 < own[2]
    # the list of v into w without a visit to the host: directly behind a surface step, and on the other stream than the edit
    # of v of the step before (the download between the steps orders that pair)
    for form, edit, a in (("devB", None, dict(which=SURFACE, box=None, kind="whole", closed=True, solid=True)),
                          ("devB", "devA", dict(which=ALL, box=cut, kind="cut", closed=False, solid=False))):
        if edit:
            w.emit(("fillBoxes", edit, dict(items=np.array([[1, 1, 1, 2, 2, 2]], np.uint32), solid=False)))
        w.emit(("listToSecond", form, dict(a, n=len(voxel_list(m.s["v"], a)))))
    # a list with a large total, then one of a small box: the second window is the second pass's
    w.emit(lists("host", ALL, None, "whole", False, 0, 399))
    w.emit(lists("host", SURFACE, [1, 1, 1, 3, 3, 3], "cut", True, 0, 399, closed=False))


def _generate(seed, depth, steps):
    """PROLOGUE, the scripted conditions, this program's stretch of the two pair walks, its share of TOUR, then seeded steps"""
    w = _Writer(seed, depth)
    index = COMMITTED.index((seed, depth)) if (seed, depth) in COMMITTED else 0
    for step in PROLOGUE:
        w.emit(step)
    _scripted(w)
    for family in _share(STAGE_WALK, index, len(COMMITTED)):
        w.one(family, "host", tries=3, pad=False)
    for family in _share(PACK_WALK, index, len(COMMITTED)):
        w.one(family, "host", tries=1, pad=False)
    for family in _share(SURFACE_WALK, index, len(COMMITTED)):
        w.one(family, None, tries=3, pad=False)
    # depths 2 .. 5 run the whole tour in every program; at 64^3, where a program is short, the three seeds share it
    share = 3 if depth >= 6 else 1
    tour = [TOUR[i] for i in w.rng.permutation(len(TOUR)) if i % share == index % share]
    for family, op, form in tour:
        w.one(family, form, op)
    names = list(FAMILIES)
    while len(w.out) < steps:
        w.one(names[int(w.rng.integers(0, len(names)))])
    return w.out, w.seen


@functools.lru_cache(maxsize=None)
def _program(seed, depth, steps):
    steps, seen = _generate(seed, depth, steps)
    return tuple(steps), tuple(seen)


def program(seed, depth, steps=None):
    """the deterministic list of steps of a seed: the same on every machine (np.random.default_rng, no hashing)"""
    return list(_program(seed, depth, STEPS[depth] if steps is None else steps)[0])


def replay(seed, depth, upto, fault=None):
    """(the mirror after the steps [0, upto) of the committed program, those steps): where the next person starts"""
    prefix = program(seed, depth)[:upto]
    m = Mirror(depth, fault)
    for step in prefix:
        m.apply(step)
    return m, prefix


def run(steps, depth, fault=None):
    """what every step of a program observes on the mirror: [(own observable, download of v, of w, scratch of v, of w, whether a
    voxel changed, the staging block of v alone)]"""
    m = Mirror(depth, fault)
    seen = []
    for step in steps:
        try:
            own = m.apply(step)
        except (IndexError, ValueError):
            if fault is None:
                raise
            break            # the faulty volume no longer fits the step's arguments: what was seen up to here is all there is
        seen.append((own, m.seen_download("v"), m.s["w"], m.scratch_bytes("v"), m.scratch_bytes("w"), m.changed, m.s["stage_v"]))
    return seen


@functools.lru_cache(maxsize=None)
def run_committed(seed, depth, fault=None):
    """run() of a committed program, computed once; the arrays in it are shared: read only"""
    if fault is None:
        return _program(seed, depth, STEPS[depth])[1]            # what the generator's own mirror saw: run() gives the same
    return tuple(run(program(seed, depth), depth, fault))


def same_value(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b
