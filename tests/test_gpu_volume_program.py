"""One pair of VoxelVolumes kept alive through a seeded program of mixed calls (tests/volume_program.py): after EVERY step
the step's own result, the download of both volumes and editScratchBytes of both are held to the numpy mirror, bit for bit.
A fresh volume's scratch is very often zeroed memory, so only a long-lived one can tell a kernel that resets its scratch
from one that relies on finding it clean.  volume_program.replay(seed, depth, upto) rebuilds the prefix of a failure."""
import ctypes as C

import numpy as np
import pytest

import volume_program as P
from volume_support import Stream, committed, differing, expected_nodes, same

pytestmark = pytest.mark.gpu


class Machine:
    """the device side of a program: the two volumes, the snapshots and the two streams"""

    def __init__(self, depth, streams):
        import cpuvoxelraycaster_amd as vrc
        self.vrc, self.capi, self.L = vrc, vrc.capi, vrc.capi.load()
        self.depth, self.S = depth, 1 << depth
        self.v, self.w = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
        self.clone = self.delta = self.labels = self.stream = None
        self.other = vrc.VoxelVolume(depth + 1)                       # the volume of another depth
        self.streams = {"host": None, "dev0": None, "devA": streams[0], "devB": streams[1]}
        self.kept = []                                                # device buffers live until the program ends

    def up(self, array):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        self.kept.append(t)
        return t

    def out(self, n_bytes):
        import torch
        t = torch.zeros(max(16, n_bytes), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.kept.append(t)
        return t

    def guarded(self, n_words):
        """an output buffer of the test's own, every 32-bit word of it the guard"""
        import torch
        t = torch.full((n_words,), P.GUARD, dtype=torch.int32, device="cuda").view(torch.uint8)
        torch.cuda.synchronize()
        self.kept.append(t)
        return t

    def window(self, t, form, skew, per, n):
        """the n records of `per` words that begin `skew` bytes into a guarded buffer; every word around them is still the guard"""
        words = self.down(t, form, np.uint32, t.numel() // 4)
        at = skew // 4
        assert np.all(words[:at] == P.GUARD) and np.all(words[at + per * n:] == P.GUARD), "the guard around the window was written"
        return words[at:at + per * n].reshape(n, per).copy()

    def down(self, t, form, dtype, n):
        if self.streams[form] is not None:
            self.L.vrc_stream_synchronize(0, self.streams[form])
        else:
            import torch
            torch.cuda.synchronize()
        return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].view(dtype).copy()

    def columns(self, records):
        """the records of a profile, from either memory kind, in the model's terms"""
        import columns_model
        if records.dtype.names is None:
            records = np.ascontiguousarray(records, np.uint32).view(self.capi.COLUMN_DTYPE)[..., 0]
        out = np.zeros(records.shape, columns_model.COLUMN_DTYPE)
        for name in columns_model.COLUMN_DTYPE.names:
            out[name] = records[name]
        return out

    def refused(self, call):
        with pytest.raises(self.vrc.VrcError):
            call()
        return "refused"

    def run(self, step):
        family, form, a = step
        vrc, capi, v, w, st = self.vrc, self.capi, self.v, self.w, self.streams[form]
        host = form == "host"
        if family in ("setVoxels", "fillBoxes", "fillSpheres"):
            if host:
                getattr(v, family)(a["items"], a["solid"])
            else:
                getattr(v, family + "Device")(len(a["items"]), self.up(a["items"]).data_ptr(), a["solid"], st)
        elif family == "fillCapsules":
            if host:
                v.fillCapsules(a["items"], a["solid"])
            else:
                v.fillCapsulesDevice(len(a["items"]), self.up(a["items"]).data_ptr(), a["solid"], st)
        elif family == "rasterMesh":
            if host:
                v.rasterMesh(a["items"], a["op"], a["solid"])
            else:
                v.rasterMesh((len(a["items"]), self.up(a["items"]).data_ptr()), a["op"], a["solid"], device=True, stream=st)
        elif family in P.AT_HITS:
            out = None
            if family == "fillSpheresAtHits":
                if host:
                    v.fillSpheresAtHits(a["hits"], a["radius"], a["solid"])
                else:
                    v.fillSpheresAtHitsDevice(len(a["hits"]), self.up(a["hits"]).data_ptr(), a["radius"], a["solid"], st)
            elif host:
                v.strokeAtHits(a["hits"], a["radius"], a["solid"], a["max_gap"])
            else:
                v.strokeAtHitsDevice(len(a["hits"]), self.up(a["hits"]).data_ptr(), a["radius"], a["solid"], a["max_gap"], st)
            if a["then"] is not None:                                 # host memory, NULL stream, right behind the brush
                kind, items = a["then"]
                out = v.setVoxels(items, True) if kind == "setVoxels" else v.getVoxels(items)
            return out
        elif family == "xorMesh":
            if host:
                v.xorMesh(a["tris"])
            else:
                v.xorMesh((len(a["tris"]), self.up(a["tris"]).data_ptr()), device=True, stream=st)
        elif family == "copyRegion":
            v.copyRegion(w, a["src_lo"], a["size"], a["dst_lo"], a["op"], st)
        elif family == "stampAffine":
            v.stampAffine(w, vrc.make_affine(a["m"], a["t"]), a["lo"], a["hi"], a["op"], st)
        elif family == "fillRandom":
            capi.check(self.L.vrc_cells_fill_random(v._h, a["seed"], a["threshold"], capi.ptr(None if a["box"] is None else np.array(a["box"], np.uint32)),
                                                    a["op"], capi.ptr(st)))
        elif family == "applyDelta":
            v.applyDelta(self.delta, st)
        elif family == "unpack":
            v.unpack(self.up(self.stream) if a["device"] else self.stream)
        elif family in ("cellStepDst", "cellStepSrc"):
            src, dst = (w, v) if family == "cellStepDst" else (v, w)
            src.cellStep(a["birth"], a["survive"], a["neighbours"], bool(a["outside"]), dst, stream=st)
        elif family == "columnProfile":
            U, V = P.rect_shape(a["rect"], self.S)
            if U * V == 0:                                            # an empty rect is refused, in either memory kind
                t = self.out(16)
                return self.refused(lambda: v.columnProfile(a["direction"], a["rect"]) if host else v.columnProfileDevice(a["direction"], t.data_ptr(), a["rect"], st))
            if host:
                return self.columns(v.columnProfile(a["direction"], a["rect"]))
            t = self.out(16 * U * V)                                  # a buffer of the test's own
            v.columnProfileDevice(a["direction"], t.data_ptr(), a["rect"], st)
            return self.columns(self.down(t, form, np.uint32, 4 * U * V).reshape(U, V, 4))
        elif family == "fillColumns":
            if host:
                v.fillColumns(a["axis"], a["lo"], a["hi"], a["rect"], a["op"])
            else:
                maps = [self.up(q).data_ptr() if np.ndim(q) else None for q in (a["lo"], a["hi"])]
                consts = [0 if np.ndim(q) else int(q) for q in (a["lo"], a["hi"])]
                v.fillColumnsDevice(a["axis"], maps[0], consts[0], maps[1], consts[1], a["rect"], a["op"], st)
        elif family in ("selectColumnsDst", "selectColumnsSrc"):
            src, dst = (w, v) if family == "selectColumnsDst" else (v, w)
            src.selectColumns(a["direction"], a["lo"], a["hi"], a["of"], dst, a["op"], st)
        elif family == "floodRegion":
            return int(v.flood(w, a["connectivity"], a["through_empty"]).reached)
        elif family == "floodMedium":
            return int(w.flood(v, a["connectivity"], a["through_empty"]).reached)
        elif family == "keepConnected":
            debris = v.keepConnected(a["anchors"], a["connectivity"])
            out = debris.download()
            debris.close()
            return out
        elif family == "dilate":
            v.dilate(a["r"])
        elif family == "erode":
            v.erode(a["r"], a["open_border"])
        elif family == "select":
            if host:
                self.labels.select(a["keep"], v, a["op"])
            else:
                self.labels.selectDevice(self.up(a["keep"]).data_ptr(), v, a["op"], st)
        elif family == "place":
            self.labels.place(a["offsets"], v, a["op"], a["keep"])
        elif family == "solidCount":
            return v.solidCount()
        elif family == "getVoxels":
            if host:
                return v.getVoxels(a["items"])
            n = len(a["items"])
            t = self.out(n)
            v.getVoxelsDevice(n, self.up(a["items"]).data_ptr(), t.data_ptr(), st)
            return self.down(t, form, np.uint8, n)
        elif family == "countBoxes":
            if host:
                return v.countBoxes(a["items"])
            n = len(a["items"])
            t = self.out(8 * n)
            v.countBoxesDevice(n, self.up(a["items"]).data_ptr(), t.data_ptr(), st)
            return self.down(t, form, np.uint64, n)
        elif family in ("surface", "rects"):
            count, window, extract = ((v.surfaceCount, v.surfaceFaces, v.extractSurfaceDevice) if family == "surface" else
                                      (v.rectCount, v.surfaceRects, v.extractRectsDevice))
            if host:
                return count(a["closed"]), window(a["closed"], a["first"], a["capacity"])
            t, total = self.out(16 * a["capacity"]), self.out(8)
            if a.get("order") == "voxels_behind":
                # the same, with a voxelCount behind the extraction: it rewrites the offsets block the two families share
                q = a["behind"]
                extract(capi.VRC_SURFACE_FACES, a["first"], a["capacity"], t.data_ptr(), total.data_ptr(), a["closed"], st)
                counts = v.voxelCount(q["op"], q["box"], q["closed"])
            elif a.get("order") == "extract_first":
                # nothing between the two calls: the extraction is still on its stream when the count of the OTHER `closed`,
                # synchronous on the NULL stream, comes to rewrite the block they share
                extract(capi.VRC_SURFACE_FACES, a["first"], a["capacity"], t.data_ptr(), total.data_ptr(), a["closed"], st)
                counts = count(not a["closed"])
            else:
                counts = count(a["closed"])
                extract(capi.VRC_SURFACE_FACES, a["first"], a["capacity"], t.data_ptr(), total.data_ptr(), a["closed"], st)
            T = int(self.down(total, form, np.uint64, 1)[0])
            n = max(0, min(a["capacity"], T - a["first"]))
            return counts, self.down(t, form, np.uint32, 4 * n).reshape(n, 4), T
        elif family == "voxels":
            if host:
                return v.voxelCount(a["op"], a["box"], a["closed"]), v.voxels(a["op"], a["box"], a["neighbours"], a["closed"], a["first"], a["capacity"])
            fmt, per = (capi.VRC_VOXELS_NEIGHBOURS, 4) if a["neighbours"] else (capi.VRC_VOXELS_XYZ, 3)
            t, total = self.guarded(a["skew"] // 4 + per * a["capacity"] + 8), self.out(8)
            args = (a["op"], fmt, a["first"], a["capacity"], t.data_ptr() + a["skew"], total.data_ptr(), a["box"], a["closed"], st)
            if a["order"] == "count_first":
                counts = v.voxelCount(a["op"], a["box"], a["closed"])
                v.extractVoxelsDevice(*args)
            else:
                # nothing between the two calls: the extraction is still on its stream when a synchronous count on the NULL stream
                # -- of another `which`, or the surface calls' -- comes to the block they all share
                v.extractVoxelsDevice(*args)
                counts = v.voxelCount((a["op"] + a["shift"]) % 3, a["box"], a["closed"]) if a["order"] == "extract_first" else v.surfaceCount(a["closed"])
            T = int(self.down(total, form, np.uint64, 1)[0])
            return counts, self.window(t, form, a["skew"], per, P.window_of(a["first"], a["capacity"], T)), T
        elif family == "listToSecond":
            # extraction and setVoxelsDevice on ONE stream; the list never visits the host, its length is the mirror's
            n = a["n"]
            t = self.guarded(3 * n + 8)
            v.extractVoxelsDevice(a["which"], capi.VRC_VOXELS_XYZ, 0, n, t.data_ptr(), None, a["box"], a["closed"], st)
            w.setVoxelsDevice(n, t.data_ptr(), a["solid"], st)
            self.window(t, form, 0, 3, n)
        elif family == "pack":
            packed = v.pack(device=not host)
            self.stream = bytes(packed.tobytes() if host else packed.cpu().numpy().tobytes())
            assert v.packInfo().bytes == len(self.stream)
            return self.stream
        elif family == "diff":
            if self.delta is not None:
                self.delta.close()
            self.delta = self.clone.diff(v)
            import delta_model
            records = self.delta.records()
            got = np.zeros(len(records), delta_model.RECORD_DTYPE)
            got["word"], got["bits"] = records["word"], records["bits"]
            return got, delta_model.stats_tuple(self.delta.stats)
        elif family == "components":
            labels = v.labelComponents(a["connectivity"])
            out = labels.components()
            labels.close()
            return out
        elif family == "distanceAt":
            field = v.distanceField(a["to_empty"], a["outside"])
            out = field.at(a["items"])
            field.close()
            return out
        elif family == "commit":
            return committed(v)
        elif family == "refuseOp":
            return self.refused(lambda: v.copyRegion(w, (0, 0, 0), (1, 1, 1), (0, 0, 0), 7))
        elif family == "refusePack":
            n = int(v.packInfo().bytes)
            buf, info = np.zeros(n, np.uint8), capi.PackInfo()
            return self.refused(lambda: capi.check(self.L.vrc_pack_volume(v._h, capi.ptr(buf), n - 1, C.byref(info), capi.VRC_MEM_HOST)))
        elif family == "refuseUnpack":
            return self.refused(lambda: v.unpack(a["data"]))
        elif family == "refuseDelta":
            return self.refused(lambda: v.deltaFromRecords(a["records"]))
        elif family == "refuseDepth":
            return self.refused(lambda: v.flood(self.other))
        elif family == "refuseMesh":
            tris = P.box_mesh([0, 0, 0], [1, 1, 1])
            return self.refused(lambda: capi.check(self.L.vrc_volume_xor_mesh(v._h, len(tris), capi.ptr(tris), 7, None)))
        elif family == "refuseRaster":
            return self.refused(lambda: v.rasterMesh(P.clipped_raster_triangles(self.S), 2, True))
        elif family == "refuseStroke":
            return self.refused(lambda: v.strokeAtHits(P.hits_of([[0, 0, 0]], self.S, miss_every=2), (1 << 13) + 1, True))
        elif family == "refuseProfile":
            return self.refused(lambda: v.columnProfile(6))
        elif family == "refuseFillAxis":
            return self.refused(lambda: v.fillColumns(3, 0, self.S))
        elif family == "refuseSelect":
            return self.refused(lambda: w.selectColumns(-1, 0, 1, 1, v))
        elif family == "refuseSelectSame":
            return self.refused(lambda: v.selectColumns(0, 0, 1, 1, v))
        elif family == "refuseSelectDepth":
            return self.refused(lambda: self.other.selectColumns(0, 0, 1, 1, v))
        elif family == "refuseVoxels":
            return self.refused(lambda: v.voxelCount(3))
        elif family == "refuseVoxelsAligned":
            t = self.guarded(16)
            out = self.refused(lambda: v.extractVoxelsDevice(0, capi.VRC_VOXELS_NEIGHBOURS, 0, 2, t.data_ptr() + 8, None))
            self.window(t, "dev0", 0, 4, 0)                           # refused, and not written
            return out
        elif family == "cloneSecond":
            w.close()
            self.w = v.clone()
        elif family == "recreateSecond":
            w.close()
            self.w = vrc.VoxelVolume(self.depth)
            capi.check(self.L.vrc_cells_fill_random(self.w._h, a["seed"], a["threshold"], None, P.OR, None))
        elif family == "snapshotLabels":
            if self.labels is not None:
                self.labels.close()
            self.labels = v.labelComponents(a["connectivity"])
            return self.labels.count
        elif family == "snapshotClone":
            if self.clone is not None:
                self.clone.close()
            self.clone = v.clone()
        else:
            raise ValueError(family)
        return None

    def close(self):
        # not the order of creation: the snapshots' source first, the second volume last
        for h in (self.v, self.delta, self.other, self.labels, self.clone, self.w):
            if h is not None:
                h.close()


def plain(value):
    """a library result in the mirror's terms"""
    if isinstance(value, np.ndarray) and value.dtype.names is not None and "voxels" in value.dtype.names and "first" in value.dtype.names:
        import components_model
        out = np.zeros(len(value), components_model.RECORD)
        for name in components_model.RECORD.names:
            out[name] = value[name]
        return out
    if isinstance(value, (tuple, list)):
        return tuple(plain(q) for q in value)
    return value


def brief(q):
    """an argument for a failure's message: long arrays by their shape, replay() has them in full"""
    if isinstance(q, np.ndarray):
        return q.tolist() if q.dtype.names is None and q.size <= 24 else "array%s" % (q.shape,)
    if isinstance(q, (bytes, bytearray)):
        return "%d bytes" % len(q)
    return tuple(brief(e) for e in q) if isinstance(q, tuple) else q


def rows(value):
    if isinstance(value, np.ndarray):
        if value.dtype.names is not None:
            return [tuple(np.asarray(r[name]).tolist() for name in value.dtype.names) for r in value]
        return value.tolist()
    if isinstance(value, tuple):
        return [rows(q) for q in value]
    return list(value) if isinstance(value, bytes) else [value]


@pytest.mark.parametrize("seed,depth", P.COMMITTED)
def test_program(built, seed, depth):
    steps = P.program(seed, depth)
    mirror = P.Mirror(depth)
    with Stream() as a, Stream() as b:
        machine = Machine(depth, (a, b))
        try:
            for i, step in enumerate(steps):
                where = dict(seed=seed, depth=depth, step=i, record=(step[0], step[1], {k: brief(q) for k, q in step[2].items()}))
                want = mirror.apply(step)
                got = plain(machine.run(step))
                if step[0] == "commit":
                    want = expected_nodes(want, depth)
                    assert same(got, want), (where, got.shape, want.shape, differing(got.view(np.uint64).tolist(), want.view(np.uint64).tolist()))
                elif want is not None:
                    assert P.same_value(got, plain(want)), (where, differing(rows(got), rows(want)))
                for name, volume in (("v", machine.v), ("w", machine.w)):
                    seen, held = volume.download(), mirror.s[name]
                    assert np.array_equal(seen, held), (where, name, differing(seen.reshape(-1).tolist(), held.reshape(-1).tolist()))
                    assert volume.editScratchBytes() == mirror.scratch_bytes(name), (where, name, volume.editScratchBytes(), mirror.scratch_bytes(name))
            v, vol = machine.v, mirror.s["v"]
            end = dict(seed=seed, depth=depth, step="after the last of %d" % len(steps))
            stream = v.pack()
            other = machine.vrc.VoxelVolume.fromPacked(stream)
            again, want = other.pack().tobytes(), P.pack_model.pack(vol, depth)
            other.close()
            assert again == stream.tobytes(), (end, "pack(unpack(pack(v)))", differing(list(again), list(stream.tobytes())))
            assert stream.tobytes() == want, (end, "pack(v)", differing(list(stream.tobytes()), list(want)))
            got, nodes = committed(v), expected_nodes(vol, depth)
            assert same(got, nodes), (end, "commit", got.shape, nodes.shape, differing(got.view(np.uint64).tolist(), nodes.view(np.uint64).tolist()))
        finally:
            machine.close()
