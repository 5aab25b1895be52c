"""The table "Ordering of the volume's entry points"  as data: one Record per entry point of a row that touches
the device and waits for, or is recorded as an edit of, a volume.  A record holds what the row says -- the stream, the
volumes the call waits for by role and in which memory forms, the volume it is recorded as an edit of, whether it is
synchronous -- and two callables:

  run(e)    a generator that issues the call on the device.  Up to its first yield it prepares what does not belong to the
            call (lists uploaded, snapshots taken, result buffers); between the first and the second yield it makes the ONE
            call under test, in e's memory form on e.stream; after the second yield -- the test has synchronised -- it
            yields the call's result.  e is an Env: e.vol[role] are the subject volumes.
  model(c)  the same result from the numpy models: c[role] are the subjects' contents when the call runs.  It returns
            (out, written): out is what run yields, written[role] the new content of every volume the call writes.

Subjects are 16^3 fields (the levels calls have a destination two depths down and one up).  The late edit of a test is
`edit(role)`: a box of voxels set by vrc_volume_set_voxels.  outcome() is what a test can observe at the end -- the result
and every subject's content -- with the call ordered behind the edit, and mistimed() the same had the call run before the
edit landed; test_ordering_cases_host.py holds every record to outcome != mistimed, on the CPU, from the models alone.
No GPU and no built library is needed to import this module."""
import functools

import numpy as np

import cells_model
import columns_model
import components_model
import contact_model
import delta_model
import distance_model
import fall_model
import flood_model
import fracture_model
import levels_model
import morph_model
import pack_model
import raster_model
import rect_model
import rigid_model
import stamp_model
import stroke_model
import surface_model
import travel_model
import volume_program
import voxelize_model
import voxels_model
from volume_support import affine_records, all_coordinates, expected_nodes

HOST, DEVICE = "host", "device"
BOTH = (HOST, DEVICE)
ANDNOT = stamp_model.ANDNOT
DEPTH, S = 4, 16


# ---- the subjects and the late edit ------------------------------------------------------------------------------

def field(seed, depth=DEPTH, density=0.37):
    size = 1 << depth
    out = (np.random.default_rng(seed).random((size, size, size)) < density).astype(np.uint8)
    out.setflags(write=False)
    return out


def edit_voxels(size):
    """the late edit: the voxels of a box with odd bounds, no face of the volume on x, set solid"""
    x, y, z = np.mgrid[size // 16:size - size // 16, 3 * size // 16:12 * size // 16, 5 * size // 16:11 * size // 16]
    return np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.uint32)


def edited(vol):
    return volume_program.voxels(vol, edit_voxels(vol.shape[0]), 1)


# ---- what run() gets -----------------------------------------------------------------------------------------------

class Env:
    """the device side of one case: the subject volumes, the memory form and the stream of the call under test, and the lists
    and result buffers in that form"""

    def __init__(self, vol, form, stream, window=None):
        import cpuvoxelraycaster_amd as vrc
        self.vrc, self.capi, self.L = vrc, vrc.capi, vrc.capi.load()
        self.vol, self.form, self.stream, self.window = vol, form, stream, window
        self.host = form == HOST
        self.mem = vrc.capi.VRC_MEM_HOST if self.host else vrc.capi.VRC_MEM_DEVICE
        self.alive, self.handles = [], []

    def ok(self, rc):
        self.capi.check(rc)

    def upload(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        self.alive.append(t)
        return t

    def arg(self, a):
        """a list of the call, in its memory form"""
        if a is None:
            return None
        if self.host:
            a = np.ascontiguousarray(a)
            self.alive.append(a)
            return self.capi.ptr(a)
        return self.capi.ptr(self.upload(a).data_ptr())

    def result(self, dtype, n):
        return Result(self, np.dtype(dtype), int(n))

    def snapshot(self, handle):
        self.handles.append(handle)
        return handle

    def close(self):
        for h in self.handles:
            h.close()
        self.handles, self.alive = [], []


class Result:
    """n items of dtype that the call writes, pre-filled with 0x5A bytes"""

    def __init__(self, e, dtype, n):
        self.dtype, self.n = dtype, n
        if e.host:
            self.buf = np.full(max(n * dtype.itemsize, 1), 0x5A, np.uint8)
            self.p = e.capi.ptr(self.buf)
        else:
            import torch
            self.buf = torch.full((max(n * dtype.itemsize, 1),), 0x5A, dtype=torch.uint8, device="cuda")
            self.p = e.capi.ptr(self.buf.data_ptr())

    def get(self, n=None):
        raw = self.buf if isinstance(self.buf, np.ndarray) else self.buf.cpu().numpy()
        n = self.n if n is None else n
        return raw[:n * self.dtype.itemsize].view(self.dtype).copy()


# ---- the records ---------------------------------------------------------------------------------------------------

class Record:
    def __init__(self, name, stream, waits, recorded, sync, forms, subjects, run, model, scratch=(), extractor=False):
        self.name = name                 # the C entry point
        self.stream = stream             # "caller's" or "NULL"
        self.waits = waits               # {role: the forms in which the call waits for it}
        self.recorded = recorded         # the role it is recorded as an edit of (device form only), or None
        self.sync = sync                 # "yes", "no" or "host / device"
        self.forms = forms               # the memory forms the call has; a call without a mem argument: (DEVICE,)
        self.subjects = subjects         # {role: content before anything}
        self.run, self.model = run, model
        self.scratch = scratch           # the roles whose vrc_volume_edit_scratch_bytes the call may change
        self.extractor = extractor       # run() honours e.window = (first, capacity)

    def returns_when_done(self, form):
        return self.sync == "yes" or (self.sync == "host / device" and form == HOST)

    def outcome(self, late_roles=()):
        """(out, {role: content}) with the call behind the edits of late_roles"""
        c = {role: (edited(vol) if role in late_roles else vol) for role, vol in self.subjects.items()}
        out, written = self.model(c)
        return out, {**c, **written}

    def mistimed(self, late_roles):
        """the same had the call run first and the edits landed afterwards"""
        out, written = self.model(dict(self.subjects))
        after = {**self.subjects, **written}
        return out, {role: (edited(vol) if role in late_roles else vol) for role, vol in after.items()}


def canon(x):
    """a result as nested tuples of Python integers and bytes, so that == is exact"""
    if isinstance(x, np.ndarray):
        if x.dtype.names:
            return (x.shape, x.tobytes())
        return (x.shape, np.ascontiguousarray(x).astype(np.int64).tobytes())
    if isinstance(x, dict):
        return tuple((k, canon(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    if isinstance(x, (np.integer, int)):
        return int(x)
    return x


RECORDS = []


def record(name, stream, waits, recorded, sync, forms=BOTH, subjects=None, scratch=(), extractor=False):
    def add(make):
        run, model = make()
        RECORDS.append(Record(name, stream, waits, recorded, sync, forms, subjects or {"v": field(5100)}, run, model, scratch, extractor))
        return make
    return add


def by_name():
    return {r.name: r for r in RECORDS}


V_HOST, V_BOTH = {"v": (HOST,)}, {"v": BOTH}
PAIR = {"src": BOTH, "dst": BOTH}


def pair_subjects(dst_depth=DEPTH):
    return {"src": field(5101), "dst": field(5102, dst_depth, 0.5)}


# -- the list edits: they clear what the late edit sets, so the order of the two shows ---------------------------------

def list_edit(name, items, dtype, entry, model_fn, waits=V_HOST, scratch=("v",)):
    @record(name, "caller's", waits, "v", "host / device", scratch=scratch)
    def _():
        def run(e):
            p = e.arg(np.ascontiguousarray(items, dtype))
            yield
            e.ok(entry(e)(e.vol["v"]._h, len(items), p, 0, e.mem, e.stream))
            yield
            yield None
        return run, lambda c: (None, {"v": model_fn(c["v"])})


CLEARED = np.array([[x, y, z] for x in range(0, 16, 2) for y in range(2, 14) for z in (4, 6, 7, 12)] + [[16, 0, 0]], np.uint32)
list_edit("vrc_volume_set_voxels", CLEARED, np.uint32, lambda e: e.L.vrc_volume_set_voxels, lambda v: volume_program.voxels(v, CLEARED, 0))
CLEARED_BOXES = np.array([[0, 0, 0, 8, 16, 9], [9, 5, 7, 13, 20, 16]], np.uint32)
list_edit("vrc_volume_fill_boxes", CLEARED_BOXES, np.uint32, lambda e: e.L.vrc_volume_fill_boxes, lambda v: volume_program.boxes(v, CLEARED_BOXES, 0))
CLEARED_SPHERES = np.array([[8, 8, 8, 5], [-1, 3, 14, 4]], np.int32)
list_edit("vrc_volume_fill_spheres", CLEARED_SPHERES, np.int32, lambda e: e.L.vrc_volume_fill_spheres, lambda v: volume_program.spheres(v, CLEARED_SPHERES, 0))
CAPSULES = np.array([[2, 4, 6, 13, 10, 9, 2, 0], [8, 8, 1, 8, 8, 14, 1, 0]], np.int32)
list_edit("vrc_stroke_fill_capsules", CAPSULES, np.int32, lambda e: e.L.vrc_stroke_fill_capsules,
          lambda v: stroke_model.fill_capsules(v.copy(), CAPSULES, 0))

MESH = np.ascontiguousarray(raster_model.box_mesh((3 * 64, 2 * 64, 4 * 64), (12 * 64, 13 * 64, 10 * 64)), np.int32)


@record("vrc_volume_xor_mesh", "caller's", V_BOTH, "v", "host / device", scratch=("v",))
def _():
    def run(e):
        p = e.arg(MESH)
        yield
        e.ok(e.L.vrc_volume_xor_mesh(e.vol["v"]._h, len(MESH), p, e.mem, e.stream))
        yield
        yield None
    return run, lambda c: (None, {"v": voxelize_model.xor_mesh(S, MESH, c["v"].copy())})


@record("vrc_raster_mesh", "caller's", V_HOST, "v", "host / device", scratch=("v",))
def _():
    def run(e):
        p = e.arg(MESH)
        yield
        e.ok(e.L.vrc_raster_mesh(e.vol["v"]._h, len(MESH), p, raster_model.TOUCHED, 0, e.mem, e.stream))
        yield
        yield None
    return run, lambda c: (None, {"v": raster_model.raster_mesh(S, MESH, raster_model.TOUCHED, 0, c["v"].copy())})


# -- the two brushes at hits (hits_call, written by hand) --------------------------------------------------------------

HIT_CELLS = [[x, y, z] for x in (2, 7, 8, 13) for y in (4, 9) for z in (6, 8, 13)]
HITS = volume_program.hits_of(HIT_CELLS, S)


def brush_model(v):
    centres = volume_program.hit_centres(HITS, S, False)
    return volume_program.spheres(v, np.concatenate([centres, np.full((len(centres), 1), 2, np.int64)], axis=1), 0)


def stroke_at_hits_model(v):
    centres, valid = volume_program.stroke_centres(HITS, S, False)
    return stroke_model.fill_capsules(v.copy(), stroke_model.stroke_items(centres, valid, 1, 0), 0)


@record("vrc_volume_fill_spheres_at_hits", "caller's", V_BOTH, "v", "host / device", scratch=("v",))
def _():
    def run(e):
        p = e.arg(HITS)
        yield
        e.ok(e.L.vrc_volume_fill_spheres_at_hits(e.vol["v"]._h, len(HITS), p, 2, 0, e.mem, e.stream))
        yield
        yield None
    return run, lambda c: (None, {"v": brush_model(c["v"])})


@record("vrc_stroke_fill_at_hits", "caller's", V_BOTH, "v", "host / device", scratch=("v",))
def _():
    def run(e):
        p = e.arg(HITS)
        yield
        e.ok(e.L.vrc_stroke_fill_at_hits(e.vol["v"]._h, len(HITS), p, 1, 0, 0, e.mem, e.stream))
        yield
        yield None
    return run, lambda c: (None, {"v": stroke_at_hits_model(c["v"])})


# -- the calls between two volumes: ANDNOT, so that the order of the call and an edit of dst shows -----------------------

def pair(name, call, model_fn, sync="no", forms=(DEVICE,), dst_depth=DEPTH, prepare=None):
    @record(name, "caller's", PAIR, "dst", sync, forms, pair_subjects(dst_depth))
    def _():
        def run(e):
            prepared = prepare(e) if prepare else None
            yield
            call(e, e.vol["dst"], e.vol["src"], prepared)
            yield
            yield None
        return run, lambda c: (None, {"dst": np.asarray(model_fn(c["dst"], c["src"]), np.uint8)})


HALF_LO, HALF_SIZE = (0, 0, 0), (16, 16, 9)
pair("vrc_volume_copy_region", lambda e, dst, src, _: dst.copyRegion(src, HALF_LO, HALF_SIZE, HALF_LO, ANDNOT, e.stream),
     lambda dst, src: stamp_model.stamp(dst, src, *stamp_model.IDENTITY, HALF_LO, HALF_SIZE, ANDNOT))
pair("vrc_volume_stamp_affine", lambda e, dst, src, _: dst.stampAffine(src, e.vrc.make_affine(*stamp_model.IDENTITY), None, None, ANDNOT, e.stream),
     lambda dst, src: stamp_model.stamp(dst, src, *stamp_model.IDENTITY, (0, 0, 0), (S, S, S), ANDNOT))
BIRTH, SURVIVE = sum(1 << c for c in range(9, 27)), sum(1 << c for c in range(6, 27))
pair("vrc_cells_step", lambda e, dst, src, _: src.cellStepDevice(dst, BIRTH, SURVIVE, None, 26, False, e.stream),
     lambda dst, src: cells_model.step(src, BIRTH, SURVIVE, 26, 0)[0])
pair("vrc_columns_select", lambda e, dst, src, _: src.selectColumns(4, 1, 3, columns_model.SOLID, dst, ANDNOT, e.stream),
     lambda dst, src: columns_model.select(dst, src, 4, 1, 3, columns_model.SOLID, ANDNOT))
ANY_LO, ANY_HI = levels_model.count_range("any", 2)
pair("vrc_levels_reduce", lambda e, dst, src, _: src.reduceInto(dst, ANY_LO + 20, ANY_HI, ANDNOT, e.stream),
     lambda dst, src: levels_model.reduce(dst, src, ANY_LO + 20, ANY_HI, ANDNOT), dst_depth=DEPTH - 2)
pair("vrc_levels_expand", lambda e, dst, src, _: src.expandInto(dst, ANDNOT, e.stream),
     lambda dst, src: levels_model.expand(dst, src, ANDNOT), dst_depth=DEPTH + 1)
ELEMENT = morph_model.line(0, 0, 1)              # two offsets: K keeps about 60 % of a field at 37 %


def morph_call(e, dst, src, p):
    e.ok(e.L.vrc_morph_apply(dst._h, src._h, morph_model.DILATE, morph_model.SOLID, len(ELEMENT), p, None, 0, ANDNOT, e.mem, e.stream))


pair("vrc_morph_apply", morph_call, lambda dst, src: morph_model.apply(dst, src, morph_model.DILATE, ELEMENT, op=ANDNOT),
     sync="host / device", forms=BOTH, prepare=lambda e: e.arg(np.ascontiguousarray(ELEMENT, np.int32)))


# -- the readers on the caller's stream -------------------------------------------------------------------------------

QUERY_XYZ = np.random.default_rng(5103).integers(0, S + 1, (2 * 256 + 7, 3)).astype(np.uint32)
QUERY_BOXES = np.array([[0, 0, 0, S, S, S], [1, 1, 1, S - 1, S - 1, S - 1], [2, 4, 6, 9, 5, 16]], np.uint32)


def reader(name, role, run, model_fn, sync="host / device", scratch=(), subjects=None, extractor=False, recorded=None):
    @record(name, "caller's", {role: BOTH}, recorded, sync, BOTH, subjects or {role: field(5100)}, scratch, extractor)
    def _():
        return run, lambda c: (model_fn(c[role]), {})


def get_voxels_run(e):
    p, out = e.arg(QUERY_XYZ), e.result(np.uint8, len(QUERY_XYZ))
    yield
    e.ok(e.L.vrc_volume_get_voxels(e.vol["v"]._h, len(QUERY_XYZ), p, out.p, e.mem, e.stream))
    yield
    yield out.get()


def count_boxes_run(e):
    p, out = e.arg(QUERY_BOXES), e.result(np.uint64, len(QUERY_BOXES))
    yield
    e.ok(e.L.vrc_volume_count_boxes(e.vol["v"]._h, len(QUERY_BOXES), p, out.p, e.mem, e.stream))
    yield
    yield out.get()


reader("vrc_volume_get_voxels", "v", get_voxels_run, lambda v: volume_program.get_voxels(v, QUERY_XYZ), scratch=("v",))
reader("vrc_volume_count_boxes", "v", count_boxes_run, lambda v: volume_program.count_boxes(v, QUERY_BOXES), scratch=("v",))


def profile_run(e):
    out = e.result(columns_model.COLUMN_DTYPE, S * S)
    yield
    e.ok(e.L.vrc_columns_profile(e.vol["v"]._h, 3, None, out.p, e.mem, e.stream))
    yield
    yield out.get().reshape(S, S)


reader("vrc_columns_profile", "v", profile_run, lambda v: columns_model.profile(v, 3))


def counts_run(e):
    out = e.result(np.uint32, (S >> 2) ** 3)
    yield
    e.ok(e.L.vrc_levels_counts(e.vol["src"]._h, 2, out.p, e.mem, e.stream))
    yield
    yield out.get().reshape(S >> 2, S >> 2, S >> 2)


reader("vrc_levels_counts", "src", counts_run, lambda v: levels_model.counts(v, 2))

# the three extractors: a window whose cuts lie inside the list, so that a shifted list shows
WINDOW = (37, 300)
SECOND_WINDOW = (5, 123)               # of the second of two extractions back to back


def extractor(name, per, call, model_fn):
    def run(e):
        first, capacity = e.window or WINDOW
        out, total = e.result(np.uint32, capacity * per), e.result(np.uint64, 1)
        yield
        e.ok(call(e, e.vol["v"]._h, first, capacity, out.p, total.p))
        yield
        count = int(total.get()[0])
        n = max(0, min(capacity, count - first))
        yield count, out.get(n * per).reshape(n, per)

    def model(c, window=None):
        first, capacity = window or WINDOW
        records = model_fn(c["v"])
        return (len(records), np.asarray(records[first:first + capacity], np.uint32)), {}

    RECORDS.append(Record(name, "caller's", V_BOTH, "v", "host / device", BOTH, {"v": field(5100)}, run, model, ("v",), True))


extractor("vrc_volume_extract_surface", 4, lambda e, v, first, capacity, out, total: e.L.vrc_volume_extract_surface(
    v, 1, e.capi.VRC_SURFACE_FACES, first, capacity, out, total, e.mem, e.stream), lambda v: surface_model.faces(v, True))
extractor("vrc_extract_rects", 4, lambda e, v, first, capacity, out, total: e.L.vrc_extract_rects(
    v, 1, e.capi.VRC_SURFACE_FACES, first, capacity, out, total, e.mem, e.stream), lambda v: rect_model.rects(v, True))
extractor("vrc_voxels_extract", 3, lambda e, v, first, capacity, out, total: e.L.vrc_voxels_extract(
    v, e.capi.VRC_VOXELS_ALL, 1, None, e.capi.VRC_VOXELS_XYZ, first, capacity, out, total, e.mem, e.stream),
    lambda v: voxels_model.voxels_dense(v, voxels_model.ALL, None, True, False))


# -- the synchronous calls on the NULL stream -------------------------------------------------------------------------

def null_reader(name, role, call, model_fn, scratch=(), forms=(DEVICE,), subjects=None):
    @record(name, "NULL", {role: BOTH}, None, "yes", forms, subjects or {role: field(5100)}, scratch)
    def _():
        def run(e):
            yield
            got = call(e, e.vol[role])
            yield
            yield got(e) if callable(got) else got
        return run, lambda c: (model_fn(c[role]), {})


def cloned(e, v):
    other = e.snapshot(v.clone())
    return lambda e: other.download()


null_reader("vrc_volume_clone", "src", cloned, lambda v: np.array(v), subjects={"src": field(5100)})
null_reader("vrc_volume_download", "v", lambda e, v: v.download(), lambda v: np.array(v))
null_reader("vrc_volume_solid_count", "v", lambda e, v: v.solidCount(), lambda v: int(v.sum()))
null_reader("vrc_volume_surface_count", "v", lambda e, v: v.surfaceCount(True), lambda v: surface_model.direction_counts(surface_model.faces(v, True)),
            scratch=("v",))
null_reader("vrc_rect_count", "v", lambda e, v: v.rectCount(True), lambda v: rect_model.direction_counts(rect_model.rects(v, True)), scratch=("v",))
null_reader("vrc_voxels_count", "v", lambda e, v: v.voxelCount(), lambda v: len(voxels_model.voxels_dense(v, voxels_model.ALL, None, True, False)),
            scratch=("v",))


def committed_nodes(e, v):
    svo = v.commit()
    return lambda e: (np.ascontiguousarray(svo.downloadNodes()).view(np.uint64).reshape(-1), svo.close())[0]


null_reader("vrc_volume_commit", "v", committed_nodes, lambda v: np.ascontiguousarray(expected_nodes(v, DEPTH)).view(np.uint64).reshape(-1))


def labelled(e, v):
    labels = e.snapshot(v.labelComponents(6))
    return lambda e: labels.at(all_coordinates(S)[:S ** 3])


def distances(e, v):
    dist = e.snapshot(v.distanceField())
    return lambda e: dist.download()


null_reader("vrc_volume_label_components", "medium", labelled, lambda v: components_model.label(v, 6)[0].reshape(-1))
null_reader("vrc_volume_distance_field", "medium", distances, lambda v: distance_model.field(v))
SITES = np.array([[2, 2, 2], [13, 13, 13], [4, 12, 7]], np.int32)


def fractured(e, v):
    handle, count = e.capi.C.c_void_p(), e.capi.C.c_uint64()
    e.ok(e.L.vrc_fracture_label(v._h, 6, e.capi.VRC_FLOOD_SOLID, len(SITES), e.sites, e.capi.VRC_DISTANCE_NONE, e.mem,
                                e.capi.C.byref(handle), e.capi.C.byref(count)))
    labels = e.snapshot(e.vrc.VoxelLabels(handle, int(count.value), DEPTH, 0))
    return lambda e: labels.at(all_coordinates(S)[:S ** 3])


@record("vrc_fracture_label", "NULL", {"medium": BOTH}, None, "yes", BOTH, {"medium": field(5100)})
def _():
    def run(e):
        e.sites = e.arg(SITES)
        yield
        got = fractured(e, e.vol["medium"])
        yield
        yield got(e)
    return run, lambda c: (fracture_model.label(c["medium"], SITES, 6)[0].reshape(-1), {})


def packed(e, v):
    info, bound = e.capi.PackInfo(), int(pack_model.bound(DEPTH))
    out = e.result(np.uint8, bound)
    return info, out, bound


@record("vrc_pack_volume", "NULL", V_BOTH, None, "yes", BOTH, scratch=("v",))
def _():
    def run(e):
        info, out, bound = packed(e, e.vol["v"])
        yield
        e.ok(e.L.vrc_pack_volume(e.vol["v"]._h, out.p, bound, e.capi.C.byref(info), e.mem))
        yield
        yield out.get(int(info.bytes))
    return run, lambda c: (np.frombuffer(bytes(pack_model.pack(c["v"], DEPTH)), np.uint8), {})


UNPACKED = field(5104, DEPTH, 0.3)


@record("vrc_unpack_volume", "NULL", V_BOTH, None, "yes", BOTH, scratch=("v",))
def _():
    def run(e):
        stream = np.frombuffer(bytes(pack_model.pack(UNPACKED, DEPTH)), np.uint8)
        p = e.arg(stream)
        yield
        e.ok(e.L.vrc_unpack_volume(e.vol["v"]._h, p, len(stream), e.mem))
        yield
        yield None
    return run, lambda c: (None, {"v": np.array(UNPACKED)})


def two_null(name, roles, recorded, call, model):
    subjects = {roles[0]: field(5105, DEPTH, 0.02), roles[1]: field(5100)} if name != "vrc_delta_diff" else {roles[0]: field(5100), roles[1]: field(5106)}

    @record(name, "NULL", {r: BOTH for r in roles}, recorded, "yes", (DEVICE,), subjects, scratch=(roles[0],) if recorded else ())
    def _():
        def run(e):
            yield
            got = call(e, e.vol[roles[0]], e.vol[roles[1]])
            yield
            yield got(e)
        return run, model


def flooded(e, region, medium):
    stats = region.flood(medium, 6)
    return lambda e: int(stats.reached)


def flood_model_of(c):
    region = flood_model.flood(c["medium"], c["region"], 6, False).astype(np.uint8)
    return int(region.sum()), {"region": region}


def travelled(e, seeds, medium):
    dist = e.snapshot(medium.travelField(seeds, 6))
    return lambda e: dist.download()


def diffed(e, before, after):
    delta = e.snapshot(before.diff(after))
    return lambda e: delta.records()


two_null("vrc_volume_flood", ("region", "medium"), "region", flooded, flood_model_of)
two_null("vrc_travel_field", ("seeds", "medium"), None, travelled, lambda c: (travel_model.field(c["medium"], c["seeds"], 6), {}))
two_null("vrc_delta_diff", ("before", "after"), None, diffed,
         lambda c: (delta_model.diff(delta_model.words_of(c["before"]), delta_model.words_of(c["after"]), DEPTH)[0], {}))


# -- the calls on a snapshot beside a volume --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pieces():
    """the labelled medium of the snapshot calls and what the models say of it, computed once"""
    vol = field(5107, DEPTH, 0.12)
    ids, records = components_model.label(vol, 6)
    count = len(records)
    rng = np.random.default_rng(5108)
    offsets = rng.integers(-3, 4, (count, 3)).astype(np.int32)
    keep = (np.arange(count) % 3 != 1).astype(np.uint8)
    maps = rigid_model.translation_maps(offsets)
    for a in (ids, offsets, keep):
        a.setflags(write=False)
    return vol, ids, count, offsets, keep, maps


def labels_of_pieces(e):
    from volume_support import labels_of
    return e.snapshot(labels_of(pieces()[0]))


def on_dst(name, prepare, call, model_fn, sync="host / device", forms=BOTH):
    @record(name, "caller's", {"dst": BOTH}, "dst", sync, forms, {"dst": field(5102, DEPTH, 0.5)})
    def _():
        def run(e):
            prepared = prepare(e)
            yield
            call(e, e.vol["dst"], *prepared)
            yield
            yield None
        return run, lambda c: (None, {"dst": np.asarray(model_fn(c["dst"]), np.uint8)})


on_dst("vrc_labels_select", lambda e: (labels_of_pieces(e), e.arg(pieces()[4])),
       lambda e, dst, labels, keep: e.ok(e.L.vrc_labels_select(labels._h, keep, dst._h, ANDNOT, e.mem, e.stream)),
       lambda dst: cells_model.apply_op(dst, components_model.select(pieces()[1], pieces()[4]), ANDNOT))
on_dst("vrc_fall_place", lambda e: (labels_of_pieces(e), e.arg(pieces()[4]), e.arg(pieces()[3])),
       lambda e, dst, labels, keep, offsets: e.ok(e.L.vrc_fall_place(labels._h, keep, offsets, dst._h, ANDNOT, e.mem, e.stream)),
       lambda dst: fall_model.place(pieces()[1], pieces()[3], dst, False, pieces()[4]))
on_dst("vrc_rigid_place_affine", lambda e: (labels_of_pieces(e), e.arg(pieces()[4]), e.arg(affine_records(pieces()[5]))),
       lambda e, dst, labels, keep, maps: e.ok(e.L.vrc_rigid_place_affine(labels._h, keep, maps, None, dst._h, ANDNOT, e.mem, e.stream)),
       lambda dst: rigid_model.place_affine(pieces()[1], pieces()[5], None, dst, rigid_model.ANDNOT, pieces()[4]))
SOURCE_OF_FIELD = field(5109, DEPTH, 0.05)


def field_of_source(e):
    from volume_support import volume_of
    medium = volume_of(SOURCE_OF_FIELD)
    dist = medium.distanceField()
    medium.close()
    return dist


on_dst("vrc_distance_select", lambda e: (e.snapshot(field_of_source(e)),),
       lambda e, dst, dist: dist.select(1, 6, dst, ANDNOT, e.stream),
       lambda dst: cells_model.apply_op(dst, distance_model.select(distance_model.field(SOURCE_OF_FIELD), 1, 6).astype(np.uint8), ANDNOT),
       sync="no", forms=(DEVICE,))
DELTA_RECORDS = delta_model.diff(delta_model.words_of(field(5110)), delta_model.words_of(field(5111)), DEPTH)[0]
on_dst("vrc_delta_apply", lambda e: (e.snapshot(e.vrc.VoxelDelta.fromRecords(DEPTH, DELTA_RECORDS)),),
       lambda e, dst, delta: dst.applyDelta(delta, e.stream),
       lambda dst: delta_model.dense_of(delta_model.apply(delta_model.words_of(dst), DELTA_RECORDS), DEPTH), sync="no", forms=(DEVICE,))


@record("vrc_rigid_contacts", "caller's", {"world": BOTH}, None, "host / device", BOTH, {"world": field(5112, DEPTH, 0.2)})
def _():
    def run(e):
        labels = labels_of_pieces(e)
        keep, maps = e.arg(pieces()[4]), e.arg(affine_records(pieces()[5]))
        out = e.result(e.capi.CONTACT_DTYPE, pieces()[2])
        yield
        e.ok(e.L.vrc_rigid_contacts(labels._h, keep, maps, None, e.vol["world"]._h, out.p, e.mem, e.stream))
        yield
        yield [contact_model.record_tuple(r) for r in out.get()]
    return run, lambda c: (contact_model.contacts(pieces()[1], pieces()[5], None, c["world"], pieces()[4]), {})


FALL_DIRECTION = 2                      # the value of capi.VRC_FACE_YN, towards smaller y (no library is imported up here)


@record("vrc_fall_drops", "NULL", {"fixed": BOTH}, None, "yes", BOTH, {"fixed": field(5113, DEPTH, 0.02)})
def _():
    def run(e):
        labels = labels_of_pieces(e)
        out, stats = e.result(np.int32, 3 * pieces()[2]), e.capi.FallStats()
        yield
        e.ok(e.L.vrc_fall_drops(labels._h, e.vol["fixed"]._h, FALL_DIRECTION, 0, out.p, e.mem, e.capi.C.byref(stats)))
        yield
        yield out.get().reshape(-1, 3)
    return run, lambda c: (fall_model.offsets_of(fall_model.drops(pieces()[1], c["fixed"], FALL_DIRECTION, 0), FALL_DIRECTION), {})


# -- the edits of one volume that take no list in its block -----------------------------------------------------------

RANDOM_SEED, RANDOM_THRESHOLD, RANDOM_BOX = 77, cells_model.threshold_of(0.4), np.array([0, 2, 0, 13, 16, 16], np.uint32)


@record("vrc_cells_fill_random", "caller's", V_BOTH, "v", "no", (DEVICE,))
def _():
    def run(e):
        yield
        e.ok(e.L.vrc_cells_fill_random(e.vol["v"]._h, RANDOM_SEED, RANDOM_THRESHOLD, e.capi.ptr(RANDOM_BOX), ANDNOT, e.stream))
        yield
        yield None
    return run, lambda c: (None, {"v": np.asarray(cells_model.fill_random(c["v"], RANDOM_SEED, RANDOM_THRESHOLD, tuple(int(q) for q in RANDOM_BOX), ANDNOT), np.uint8)})


FILL_LO = (np.arange(S * S, dtype=np.int32).reshape(S, S) * 7 % 11).astype(np.int32)
FILL_HI = (FILL_LO + 3 + np.arange(S, dtype=np.int32)[None, :] % 4).astype(np.int32)


@record("vrc_columns_fill", "caller's", V_BOTH, "v", "host / device")
def _():
    def run(e):
        lo, hi = e.arg(FILL_LO), e.arg(FILL_HI)
        yield
        e.ok(e.L.vrc_columns_fill(e.vol["v"]._h, 1, None, lo, 0, hi, 0, ANDNOT, e.mem, e.stream))
        yield
        yield None
    return run, lambda c: (None, {"v": columns_model.fill(c["v"], 1, FILL_LO, FILL_HI, None, ANDNOT)})
