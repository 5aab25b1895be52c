"""Holds the seeded programs of tests/volume_program.py to what they are for, on the CPU alone: the mirror is the models,
the committed seeds cover the step pairs that share a persistent block, no program idles, and each modelled hazard (a
Mirror fault switch) changes what at least one step of every depth-5 program observes."""
import numpy as np
import pytest

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
import volume_program as P
import voxelize_model
import voxels_model


def field(S, seed, density=0.4):
    return (np.random.default_rng(seed).random((S, S, S)) < density).astype(np.uint8)


def primed(depth):
    """a mirror whose two volumes hold random fields and whose snapshots exist"""
    S = 1 << depth
    m = P.Mirror(depth)
    m.s["v"], m.s["w"] = field(S, 1), field(S, 2)
    m.apply(("snapshotLabels", "host", dict(connectivity=6)))
    m.apply(("snapshotClone", "host", {}))
    m.s["v"] = field(S, 3)
    m.apply(("diff", "host", {}))
    m.apply(("pack", "host", {}))
    m.s["v"] = field(S, 4)
    return m


def test_one_step_is_the_family_model():
    depth, S = 3, 8
    rng = np.random.default_rng(5)
    for family in P.EDITS + P.QUERIES:
        for form in P._FORMS_OF.get(family, ("host",)):
            for op in (0, 1, 2):
                m = primed(depth)
                a = P._arguments(rng, family, form, m)
                if "op" in a:
                    a["op"] = (P.OR, P.ANDNOT)[op % 2] if family == "place" else op % 2 if family == "rasterMesh" else op
                if family == "strokeAtHits":
                    a["then"] = None                           # the call behind a stroke: test_one_step_refusals_lifetime_...
                v, w, ids = m.s["v"], m.s["w"], m.s["ids"]
                out = m.apply((family, form, a))
                value = 1 if a.get("solid") else 0
                want_v, want_w, want = v, w, None
                if family == "setVoxels":
                    want_v = v.copy()
                    for x, y, z in a["items"]:
                        if max(x, y, z) < S:
                            want_v[x, y, z] = value
                elif family == "fillBoxes":
                    want_v = v.copy()
                    for b in a["items"]:
                        want_v[b[0]:b[3], b[1]:b[4], b[2]:b[5]] = value
                elif family == "fillSpheres":
                    g = np.indices((S, S, S)).astype(np.int64)
                    want_v = v.copy()
                    for cx, cy, cz, r in a["items"].astype(np.int64):
                        want_v[(g[0] - cx) ** 2 + (g[1] - cy) ** 2 + (g[2] - cz) ** 2 <= r * r] = value
                elif family == "fillSpheresAtHits":
                    continue                                   # held by test_hits_name_their_cells below
                elif family == "xorMesh":
                    want_v = voxelize_model.xor_mesh(S, a["tris"], v.copy())
                elif family == "fillCapsules":
                    g = np.indices((S, S, S)).astype(np.int64)          # the rule over the whole volume, no bounding box
                    want_v = v.copy()
                    for item in a["items"].tolist():
                        if stroke_model.kept(item) and item[6] >= 0:
                            want_v[stroke_model.rule(g[0], g[1], g[2], item)] = value
                    assert any(stroke_model.kept(i) and abs(i[3 + k] - i[k]) == 12 for i in a["items"].tolist() for k in range(3))       # the crossing one
                elif family == "strokeAtHits":
                    rec = a["hits"]
                    centres = S - 1 - np.floor((rec["position"].astype(np.float64) - 1.0) * S).astype(np.int64) + ([0, 1, 0] if a["solid"] else [0, 0, 0])
                    valid = (rec["hit"] == 1) & (centres[:, 1] < S)
                    want_v = stroke_model.fill_capsules(v.copy(), stroke_model.stroke_items(centres, valid, a["radius"], a["max_gap"]), value)
                elif family == "rasterMesh":
                    want_v = raster_model.raster_mesh(S, a["items"], a["op"], a["solid"], v.copy())
                elif family == "fillColumns":
                    want_v = columns_model.fill(v, a["axis"], a["lo"], a["hi"], a["rect"], a["op"])
                    assert a["maps"] == sum(np.ndim(q) == 2 for q in (a["lo"], a["hi"])) and (form != "host" or a["maps"] >= 1)
                elif family == "selectColumnsDst":
                    want_v = columns_model.select(v, w, a["direction"], a["lo"], a["hi"], a["of"], a["op"])
                elif family == "selectColumnsSrc":
                    want_w = columns_model.select(w, v, a["direction"], a["lo"], a["hi"], a["of"], a["op"])
                elif family == "columnProfile":
                    empty = a["rect"] is not None and (a["rect"][0] >= a["rect"][2] or a["rect"][1] >= a["rect"][3])
                    want = "refused" if empty else columns_model.profile(v, a["direction"], a["rect"])
                elif family == "copyRegion":
                    m_, t_ = stamp_model.IDENTITY
                    t_ = [(a["src_lo"][k] - a["dst_lo"][k]) << 17 for k in range(3)]
                    want_v = stamp_model.stamp(v, w, m_, t_, a["dst_lo"], [a["dst_lo"][k] + a["size"][k] for k in range(3)], a["op"])
                elif family == "stampAffine":
                    want_v = stamp_model.stamp(v, w, a["m"], a["t"], a["lo"], a["hi"], a["op"])
                elif family == "fillRandom":
                    want_v = cells_model.fill_random(v, a["seed"], a["threshold"], a["box"], a["op"])
                elif family == "applyDelta":
                    want_v = delta_model.dense_of(delta_model.apply(delta_model.words_of(v), m.s["delta"]), depth)
                elif family == "unpack":
                    want_v = field(S, 3)
                elif family == "cellStepDst":
                    want_v = cells_model.step(w, a["birth"], a["survive"], a["neighbours"], a["outside"])[0]
                elif family == "cellStepSrc":
                    want_w = cells_model.step(v, a["birth"], a["survive"], a["neighbours"], a["outside"])[0]
                elif family == "floodRegion":
                    want_v = flood_model.flood_plain(w, v, a["connectivity"], a["through_empty"])
                    want = int(want_v.sum())
                elif family == "floodMedium":
                    want_w = flood_model.flood_plain(v, w, a["connectivity"], a["through_empty"])
                    want = int(want_w.sum())
                elif family == "keepConnected":
                    b = a["anchors"][0]
                    seeds = np.zeros_like(v)
                    seeds[b[0]:b[3], b[1]:b[4], b[2]:b[5]] = 1
                    want_v = flood_model.flood_plain(v, seeds, a["connectivity"])
                    want = v & (1 - want_v)
                elif family == "dilate":
                    want_v = distance_model.dilate(v, a["r"]).astype(np.uint8)
                elif family == "erode":
                    want_v = distance_model.erode(v, a["r"], a["open_border"]).astype(np.uint8)
                elif family == "select":
                    want_v = cells_model.apply_op(v, components_model.select(ids, a["keep"]), a["op"])
                elif family == "place":
                    want_v = fall_model.place(ids, a["offsets"], v, a["op"] == P.OR, a["keep"])
                elif family == "solidCount":
                    want = int(v.sum())
                elif family == "getVoxels":
                    want = np.array([v[x, y, z] if max(x, y, z) < S else 0 for x, y, z in a["items"]], np.uint8)
                elif family == "countBoxes":
                    want = np.array([v[b[0]:b[3], b[1]:b[4], b[2]:b[5]].sum() for b in a["items"]], np.uint64)
                elif family == "surface":
                    f = surface_model.faces(v, a["closed"])
                    other = form != "host" and a["order"] == "extract_first"        # the count of the other `closed` in between
                    want = (surface_model.direction_counts(surface_model.faces(v, not a["closed"]) if other else f),
                            f[a["first"]:a["first"] + a["capacity"]]) + (() if form == "host" else (len(f),))
                    if form != "host" and a["order"] == "voxels_behind":            # or a voxelCount, whose result the step carries
                        q = a["behind"]
                        want = (len(voxels_model.brute(v.tolist(), q["op"], q["box"], q["closed"])),) + want[1:]
                elif family == "rects":
                    r = rect_model.rects(v, a["closed"])
                    other = form != "host" and a["order"] == "extract_first"
                    want = (rect_model.direction_counts(rect_model.rects(v, not a["closed"]) if other else r),
                            r[a["first"]:a["first"] + a["capacity"]]) + (() if form == "host" else (len(r),))
                elif family == "voxels":
                    # the triple loop, not the dense model the mirror uses; the six surface totals are the cleared face bits
                    # of the SURFACE masks of the whole volume (vrc.h:428-429), from the same loop
                    b = voxels_model.brute(v.tolist(), a["op"], a["box"], a["closed"])
                    listed = np.ascontiguousarray(b if a["neighbours"] else b[:, :3])
                    window = listed[a["first"]:a["first"] + a["capacity"]]
                    if form == "host":
                        want = (len(b), window)
                    else:
                        assert a["skew"] in (0, 4) and not (a["skew"] and a["neighbours"])
                        behind = {"count_first": lambda: len(b),
                                  "extract_first": lambda: len(voxels_model.brute(v.tolist(), (a["op"] + a["shift"]) % 3, a["box"], a["closed"])),
                                  "surface_behind": lambda: voxels_model.cleared_face_bits(voxels_model.brute(v.tolist(), voxels_model.SURFACE, None, a["closed"]))}
                        want = (behind[a["order"]](), window, len(b))
                elif family == "listToSecond":
                    want_w = w.copy()
                    for x, y, z, _ in voxels_model.brute(v.tolist(), a["which"], a["box"], a["closed"]).tolist():
                        want_w[x, y, z] = value
                    assert a["n"] == len(voxels_model.brute(v.tolist(), a["which"], a["box"], a["closed"]))
                elif family == "pack":
                    want = pack_model.pack(v, depth)
                elif family == "diff":
                    records, stats = delta_model.diff(delta_model.words_of(field(S, 1)), delta_model.words_of(v), depth)
                    want = (records, delta_model.stats_tuple(stats))
                elif family == "components":
                    want = components_model.label(v, a["connectivity"])[1]
                elif family == "distanceAt":
                    D = distance_model.field(v, a["to_empty"], a["outside"])
                    want = np.array([D[x, y, z] for x, y, z in a["items"]], np.uint32)
                elif family == "commit":
                    want = v
                assert np.array_equal(m.s["v"], want_v) and np.array_equal(m.s["w"], want_w), (family, form, op)
                assert P.same_value(out, want), (family, form, op)
                if "op" not in a:
                    break


def test_hits_name_their_cells():
    for S in (4, 8, 32, 64):
        cells = np.indices((S, S, S)).reshape(3, -1).T
        rec = P.hits_of(cells, S, miss_every=7)
        hit = np.ones(len(cells), bool)
        hit[::7] = False
        assert np.array_equal(P.hit_centres(rec, S, False), cells[hit])
        build = cells[hit] + [0, 1, 0]
        assert np.array_equal(P.hit_centres(rec, S, True), build[build[:, 1] < S])
    m = P.Mirror(3)
    m.s["v"] = field(8, 9)
    rec = P.hits_of([[1, 2, 3], [4, 7, 4], [5, 5, 5]], 8, miss_every=3)             # record 0 is a miss
    m.apply(("fillSpheresAtHits", "devA", dict(hits=rec, radius=1, solid=True, then=None)))
    assert np.array_equal(m.s["v"], P.spheres(field(8, 9), [[5, 6, 5, 1]], 1))      # (4, 8, 4) lies outside: no neighbour


def test_one_step_refusals_lifetime_and_the_call_behind_a_brush():
    depth, S = 3, 8
    rng = np.random.default_rng(6)
    for family in P.REFUSALS:
        m = primed(depth)
        before = m.save()
        scratch = (m.scratch_bytes("v"), m.scratch_bytes("w"))
        assert m.apply((family, "host", P._arguments(rng, family, "host", m))) == "refused" and not m.changed
        assert all(m.s[k] is before[k] for k in before if k != "before_edit")          # nothing at all moved
        assert (m.scratch_bytes("v"), m.scratch_bytes("w")) == scratch
        if family == "refuseUnpack":
            a = P._arguments(rng, family, "host", m)
            assert pack_model.unpack(a["data"], depth)[0] == a["rule"]                 # the model refuses it, by that rule
    # a refused voxel call on a volume that has seen no surface or voxel call reserves no offsets block; the first real one does
    m = P.Mirror(depth)
    for family in ("refuseVoxels", "refuseVoxelsAligned"):
        assert m.apply((family, "host", {})) == "refused" and m.scratch_bytes() == 0 and not m.s["blocks_v"]
    m.apply(("voxels", "dev0", dict(op=0, box=None, closed=True, neighbours=False, first=0, capacity=4, skew=0, order="count_first", shift=1)))
    assert m.scratch_bytes() == P.surface_bytes(depth)
    for seed, deep in P.COMMITTED:
        steps = P.program(seed, deep)
        first = min(i for i, s in enumerate(steps) if s[0] in P.BLOCKS["d_surface"])
        assert {"refuseVoxels", "refuseVoxelsAligned"} <= {s[0] for s in steps[:first]}, (seed, deep)
    m = primed(depth)
    v, w = m.s["v"], m.s["w"]
    m.apply(("floodMedium", "host", dict(connectivity=6, through_empty=False)))        # w gains a flood block
    assert m.scratch_bytes("w") == P.flood_bytes(depth)
    m.apply(("cloneSecond", "host", {}))
    assert m.s["w"] is v and m.scratch_bytes("w") == 0                                 # a clone starts without scratch
    m.apply(("recreateSecond", "host", dict(seed=3, threshold=cells_model.threshold_of(0.4))))
    assert np.array_equal(m.s["w"], cells_model.random_set(3, cells_model.threshold_of(0.4), S)) and m.scratch_bytes("w") == 0
    m.s["v"] = field(S, 11)
    ids, records = components_model.label(m.s["v"], 26)
    assert m.apply(("snapshotLabels", "host", dict(connectivity=26))) == len(records) and np.array_equal(m.s["ids"], ids)
    m.apply(("snapshotClone", "host", {}))
    held = m.s["v"]
    m.apply(("fillBoxes", "host", dict(items=np.array([[0, 0, 0, S, S, S]], np.uint32), solid=False)))
    assert m.s["clone"] is held and np.array_equal(m.s["ids"], ids)                    # snapshots do not follow later edits
    # the call a brush carries behind it
    start = field(S, 12)
    cells = np.argwhere(start)[:5]
    for kind in ("setVoxels", "getVoxels"):
        m = P.Mirror(depth)
        m.s["v"] = start
        items = cells[1:].astype(np.uint32)
        out = m.apply(("fillSpheresAtHits", "devB", dict(hits=P.hits_of(cells, S, miss_every=10), radius=0, solid=False, then=(kind, items))))
        dug = P.voxels(start, cells[1:], 0)                                            # record 0 is a miss
        if kind == "setVoxels":
            assert out is None and np.array_equal(m.s["v"], start)                     # dug, then set again
        else:
            assert np.array_equal(out, np.zeros(4, np.uint8)) and np.array_equal(m.s["v"], dug)
        assert m.scratch_bytes() == max(16 * 5, (12 if kind == "setVoxels" else 13) * 4)


def test_programs_are_deterministic_and_replay_rebuilds_the_prefix():
    seed, depth = P.COMMITTED[0]
    P._program.cache_clear()
    first = P.program(seed, depth)
    P._program.cache_clear()
    again = P.program(seed, depth)
    assert len(first) == P.STEPS[depth] and all(a[:2] == b[:2] and P.same_value(tuple(a[2].values()), tuple(b[2].values())) for a, b in zip(first, again))
    # what the generator's own mirror saw, which the other tests read, is what a fresh mirror sees
    assert P.same_value(tuple(o[:5] for o in P.run_committed(seed, depth)), tuple(o[:5] for o in P.run(first, depth)))
    m, prefix = P.replay(seed, depth, 40)
    assert len(prefix) == 40 and np.array_equal(m.s["v"], P.run(first[:40], depth)[-1][1])


def adjacent(steps):
    return list(zip(steps, steps[1:]))


def test_coverage_of_the_committed_seeds():
    covered, used = set(), set()
    for seed, depth in P.COMMITTED:
        steps = P.program(seed, depth)
        seen = P.run_committed(seed, depth)
        used |= {s[0] for s in steps} | {(s[0], s[1]) for s in steps}
        for a, b in adjacent(steps):
            covered |= P.covers(a, b)
        names = [s[0] for s in steps]
        counts = [int(o[1].sum()) for o in seen]
        # d_stage: larger list then smaller list; device-memory brush at hits on a stream, then a host-memory list call
        assert any(a[0] == b[0] == "setVoxels" and a[1] == b[1] == "host" and len(a[2]["items"]) > len(b[2]["items"]) for a, b in adjacent(steps)), (seed, depth)
        assert any(a[0] == "fillSpheresAtHits" and a[1] in ("devA", "devB") and P.stages(b) and b[1] == "host" for a, b in adjacent(steps)), (seed, depth)
        # a commit follows an edit that lowered the solid count
        assert any(names[i] == "commit" and names[i - 1] in P.EDITS and counts[i - 1] < counts[i - 2] for i in range(2, len(steps))), (seed, depth)
        # a rectCount and a surfaceCount each follow an edit, with an earlier call of their family and none between
        for family in ("rects", "surface"):
            at = [i for i, n in enumerate(names) if n == family]
            assert any(any(n in P.EDITS and seen[k][5] for k, n in enumerate(names[i + 1:j], i + 1)) for i, j in zip(at, at[1:])), (seed, depth, family)
        # an xorMesh follows a refused xorMesh and one whose triangles were all clipped
        meshes = [s for s in steps if s[0] in ("xorMesh", "refuseMesh")]
        assert any(a[0] == "refuseMesh" and b[0] == "xorMesh" for a, b in adjacent(meshes)), (seed, depth)
        assert any(a[0] == "xorMesh" and a[2]["kind"] == "clipped" and b[0] == "xorMesh" and b[2]["kind"] != "clipped" for a, b in adjacent(meshes)), (seed, depth)
        # a flood with v as region follows an edit of the other volume used as medium
        assert any(a[0] in ("floodMedium", "cellStepSrc", "recreateSecond", "cloneSecond") and seen[i][5] and b[0] == "floodRegion"
                   for i, (a, b) in enumerate(adjacent(steps))), (seed, depth)
        # inside one step: a brush on a stream of the test's own with a host list edit behind it, and one with a host query
        # of voxels the brush changes; an extraction on a stream with the count behind it, for both meshes
        brushes = [s for s in steps if s[0] == "fillSpheresAtHits" and s[1] in ("devA", "devB") and s[2]["then"] is not None]
        assert any(s[2]["then"][0] == "setVoxels" for s in brushes), (seed, depth)
        good = False
        for i, s in enumerate(steps):
            if any(s is b for b in brushes) and s[2]["then"][0] == "getVoxels":
                before = P.get_voxels(seen[i - 1][1], s[2]["then"][1])
                good = good or not np.array_equal(before, seen[i][0])
        assert good, (seed, depth)
        for family in ("surface", "rects"):
            assert any(s[0] == family and s[1] in ("devA", "devB") and s[2].get("order") == "extract_first" for s in steps), (seed, depth, family)
        # the stroke at hits, whose kernel reads centre i and i + 1 in the staging block: on a stream of the test's own with a host
        # staging call as the next step; and inside one step with a host list edit behind it, and with a host query of voxels it changes
        assert any(a[0] == "strokeAtHits" and a[1] in ("devA", "devB") and P.stages(b) and b[1] == "host" for a, b in adjacent(steps)), (seed, depth)
        strokes = [(i, s) for i, s in enumerate(steps) if s[0] == "strokeAtHits" and s[1] in ("devA", "devB") and s[2]["then"] is not None]
        assert any(s[2]["then"][0] == "setVoxels" and len(s[2]["then"][1]) >= 4 for _, s in strokes), (seed, depth)
        assert any(s[2]["then"][0] == "getVoxels" and not np.array_equal(P.get_voxels(seen[i - 1][1], s[2]["then"][1]), seen[i][0]) for i, s in strokes), (seed, depth)
        # a host columnProfile directly after a larger host list edit: the records come down through a block of the call's own
        # and the volume's scratch does not move; a fillColumns with two host maps directly after one with one
        assert any(a[0] in P.ITEM_BYTES and a[1] == b[1] == "host" and b[0] == "columnProfile" and seen[i + 1][3] == seen[i][3] and
                   0 < 16 * int(np.prod(P.rect_shape(b[2]["rect"], 1 << depth))) < P.ITEM_BYTES[a[0]] * len(a[2]["items" if "items" in a[2] else "tris"])
                   for i, (a, b) in enumerate(adjacent(steps))), (seed, depth)
        assert any(a[0] == b[0] == "fillColumns" and a[1] == b[1] == "host" and (a[2]["maps"], b[2]["maps"]) == (1, 2) for a, b in adjacent(steps)), (seed, depth)
        # a rasterMesh follows a refused one and one whose triangles were all clipped
        rasters = [s for s in steps if s[0] in ("rasterMesh", "refuseRaster")]
        assert any(a[0] == "refuseRaster" and b[0] == "rasterMesh" for a, b in adjacent(rasters)), (seed, depth)
        assert any(a[0] == "rasterMesh" and a[2]["kind"] == "clipped" and b[0] == "rasterMesh" and b[2]["kind"] != "clipped" for a, b in adjacent(rasters)), (seed, depth)
        # no column call moves the scratch of either volume
        for i, s in enumerate(steps):
            if s[0] in P.OWN_BLOCK + ("selectColumnsDst", "selectColumnsSrc") and i:
                assert seen[i][3:5] == seen[i - 1][3:5], (seed, depth, i)
        # inside one step, in the offsets block the voxel lists share with the surface calls: a voxel extraction on a stream
        # with the voxelCount of another `which` behind it, one with a surfaceCount behind it, and a surface extraction with a
        # voxelCount behind it -- each count another number than the total of the extraction it follows, so that offsets gone
        # stale show in the step's own result
        streams = [(s, o[0]) for s, o in zip(steps, seen) if s[1] in ("devA", "devB") and s[0] in ("voxels", "surface")]
        assert any(s[0] == "voxels" and s[2]["order"] == "extract_first" and own[0] != own[2] for s, own in streams), (seed, depth)
        assert any(s[0] == "voxels" and s[2]["order"] == "surface_behind" and int(own[0].sum()) != own[2] > 0 for s, own in streams), (seed, depth)
        assert any(s[0] == "surface" and s[2]["order"] == "voxels_behind" and own[0] != own[2] and own[0] > 0 for s, own in streams), (seed, depth)
        # the host windows of the lists in the staging block: one directly behind a larger host list edit, one that grows the
        # block to exactly record * window, and an empty window (of a list that is not empty) that leaves the block alone
        def window_bytes(i):
            a, own = steps[i][2], seen[i][0]
            return (16 if a["neighbours"] else 12) * P.window_of(a["first"], a["capacity"], own[0])
        def prev_bytes(i):                                       # what a host list edit staged as the step before, else 0
            family, form, a = steps[i - 1]
            if family not in P.ITEM_BYTES or family not in P.EDITS or form != "host":
                return 0
            return P.ITEM_BYTES[family] * len(a["items" if "items" in a else "tris"])
        lists = [i for i, s in enumerate(steps) if s[0] == "voxels" and s[1] == "host" and i]
        for i in lists:
            assert window_bytes(i) == seen[i][0][1].nbytes, (seed, depth, i)
        assert any(0 < window_bytes(i) < prev_bytes(i) for i in lists), (seed, depth)
        grew = [i for i in lists if seen[i][6] == window_bytes(i) > seen[i - 1][6]]               # the block is now exactly the window
        assert any(seen[i][3] - seen[i - 1][3] == window_bytes(i) - seen[i - 1][6] for i in grew), (seed, depth)
        empty = [i for i in lists if window_bytes(i) == 0 < seen[i][0][0]]
        assert any(seen[i][6] == seen[i - 1][6] > 0 and seen[i][3] == seen[i - 1][3] for i in empty), (seed, depth)
        # the list of v into w on a stream, directly behind an edit of v on the other stream, and directly behind a surface step
        assert any(a[0] in P.EDITS and a[0] not in P.EDITS_OF_W and {a[1], b[1]} == {"devA", "devB"} and b[0] == "listToSecond" and seen[i][5]
                   for i, (a, b) in enumerate(adjacent(steps))), (seed, depth)
        assert any(a[0] == "surface" and b[0] == "listToSecond" for a, b in adjacent(steps)), (seed, depth)
    assert set(P.shared_pairs()) <= covered, sorted(set(P.shared_pairs()) - covered)
    assert {("d_stage", a, b) for a in ("fillCapsules", "strokeAtHits", "rasterMesh") for b in P.BLOCKS["d_stage"]} <= covered
    for form in P.FORMS[1:]:                                    # the stream-only edits: each stream occurs among them
        assert any((family, form) in used for family in P.STREAM_EDITS), form
    # every family, every op of the families that take one and every form of the list calls: at EVERY depth
    for depth in P.DEPTHS:
        steps = [s for seed in P.SEEDS[depth] for s in P.program(seed, depth)]
        # a family that takes an op (rasterMesh: a mode) and has all four forms also counts under (family, None, form)
        ran = {(s[0], op, form) for s in steps for op in (s[2].get("op"), None) for form in (s[1], None)}
        assert set(P.TOUR) <= ran, (depth, sorted(set(P.TOUR) - ran, key=str))
        assert {(family, None, form) for family in P.ALL_FORMS for form in P.FORMS} <= ran, depth
        changed = {(s[0], s[2].get("op")) for seed in P.SEEDS[depth] for s, o in zip(P.program(seed, depth), P.run_committed(seed, depth)) if o[5]}
        idle = {(f, op) for f, op, _ in P.TOUR if f in P.EDITS} - changed
        assert not idle, (depth, idle)                          # and each edit, with each op, changes a voxel there at least once
        # the voxel lists: both record formats for each `which`, every kind of box, an output that is 4- but not 8-byte aligned
        lists = [s for s in steps if s[0] == "voxels"]
        assert {(which, nb) for which in range(3) for nb in (False, True)} <= {(s[2]["op"], s[2]["neighbours"]) for s in lists}, depth
        assert set(P.BOX_KINDS) <= {s[2]["kind"] for s in lists}, depth
        assert any(s[1] != "host" and s[2]["skew"] == 4 for s in lists), depth
        for s in lists:
            box, S = s[2]["box"], 1 << depth
            if s[2]["kind"] == "cut":                           # words cut on all three axes
                assert all(q % 2 == 1 for q in box[0:2] + box[3:5]) and box[2] % 8 and box[5] % 8 and all(0 < l < h < S for l, h in zip(box[:3], box[3:])), box
            assert s[2]["kind"] != "beyond" or all(h > S for h in box[3:])
            assert s[2]["kind"] != "empty" or voxels_model.clipped(box, S) is None
            assert s[2]["kind"] != "whole" or box in (None, [0, 0, 0, S, S, S])
    assert {("d_surface", a, b) for a in P.BLOCKS["d_surface"] for b in P.BLOCKS["d_surface"]} <= covered
    assert {("d_stage", a, b) for a in P.BLOCKS["d_stage"] for b in P.BLOCKS["d_stage"] if "voxels" in (a, b)} <= covered


@pytest.mark.parametrize("seed,depth", P.COMMITTED)
def test_no_idle_program(seed, depth):
    steps = P.program(seed, depth)
    seen = P.run_committed(seed, depth)
    edits = [o[5] for s, o in zip(steps, seen) if s[0] in P.EDITS]
    queries = [P.is_empty(o[0]) for s, o in zip(steps, seen) if s[0] in P.QUERIES]
    assert len(edits) >= len(steps) // 4 and len(queries) >= len(steps) // 5
    assert sum(edits) >= 0.8 * len(edits), (sum(edits), len(edits))
    assert sum(queries) <= 0.1 * len(queries), (sum(queries), len(queries))
    for s, o in zip(steps, seen):
        if s[0] in P.REFUSALS:
            assert not o[5]                                     # a refusal leaves both volumes as they were


@pytest.mark.parametrize("fault", P.FAULTS)
@pytest.mark.parametrize("seed", P.SEEDS[5])
def test_every_fault_is_visible(seed, fault):
    # zip: where the faulty mirror could not go on (run() stops there) only the steps it did observe count
    good, bad = P.run_committed(seed, 5), P.run_committed(seed, 5, fault)
    assert any(not P.same_value(g[:5], b[:5]) for g, b in zip(good, bad)), (seed, fault)
    if fault == "unordered":
        # not through the download alone: the query behind a brush and the extraction under a count see it themselves
        own = {s[0] for s, g, b in zip(P.program(seed, 5), good, bad) if not P.same_value(g[0], b[0])}
        assert {"fillSpheresAtHits", "strokeAtHits", "surface", "rects", "voxels"} <= own, (seed, own)
        # the surface extraction by both counts that may come behind it: its own family's, and the voxel lists'
        orders = {s[2].get("order") for s, g, b in zip(P.program(seed, 5), good, bad) if s[0] == "surface" and not P.same_value(g[0], b[0])}
        assert {"extract_first", "voxels_behind"} <= orders, (seed, orders)
    if fault == "totals":
        # a host window of the lists, by itself, and nothing before it
        first = next(s for s, g, b in zip(P.program(seed, 5), good, bad) if not P.same_value(g[:5], b[:5]))
        assert first[0] == "voxels" and first[1] == "host", (seed, first[:2])
    if fault == "links":
        # the stroke itself went wrong, not a call behind it: the first step that differs is a stroke with a list edit behind it
        first = next(s for s, g, b in zip(P.program(seed, 5), good, bad) if not P.same_value(g[:5], b[:5]))
        assert first[0] == "strokeAtHits" and first[1] in ("devA", "devB") and first[2]["then"][0] == "setVoxels", (seed, first[:2])


def test_faults_show_through_the_new_families():
    """stage_tail, unordered and links on mirrors of a few steps: each new family that writes the staging block, or edits on a
    stream, shows the hazard by itself"""
    depth, S = 5, 32
    start = field(S, 21)
    caps = np.array([[i, 2, 3, i, 20, 9, 1, 0] for i in range(10)], np.int32)
    tris = raster_model.box_mesh([70, 70, 70], [900, 1000, 1100]).astype(np.int32)

    def seen(steps, fault):
        m = P.Mirror(depth, fault)
        m.s["v"], m.s["w"] = start, field(S, 22)
        return [(m.apply(step), m.seen_download("v"), m.scratch_bytes("v")) for step in steps]

    def visible(steps, fault):
        return not P.same_value(tuple(seen(steps, None)), tuple(seen(steps, fault)))

    # a longer host list, then a shorter one: the call reads the items the block still holds behind its own
    assert visible([("fillCapsules", "host", dict(items=caps, solid=False)), ("fillCapsules", "host", dict(items=caps[:2], solid=True))], "stage_tail")
    assert visible([("rasterMesh", "host", dict(items=tris, op=P.TOUCHED, solid=False)), ("rasterMesh", "host", dict(items=tris[:1], op=P.TOUCHED, solid=True))], "stage_tail")
    # the download, and the query a stroke carries, right behind an edit on a stream
    one = np.full((4, 4), 9, np.int32)
    for step in (("fillCapsules", "devA", dict(items=caps, solid=False)), ("rasterMesh", "devB", dict(items=tris, op=P.THIN, solid=False)),
                 ("fillColumns", "devA", dict(axis=0, rect=[1, 1, 5, 5], op=P.REPLACE, lo=one - 4, hi=one, maps=2)),
                 ("selectColumnsDst", "devB", dict(direction=3, lo=0, hi=2, of=columns_model.SOLID, op=P.REPLACE))):
        assert visible([step], "unordered"), step[0]
    cells = np.argwhere(start)[:40:5]
    stroke = dict(hits=P.hits_of(cells, S, miss_every=10), radius=0, max_gap=0, solid=False)
    query = [("strokeAtHits", "devA", dict(stroke, then=("getVoxels", cells[1:].astype(np.uint32))))]
    assert not P.same_value(seen(query, None)[0][0], seen(query, "unordered")[0][0]) and not seen(query, None)[0][0].any()
    # k_stroke_links reads centre i + 1 after the list edit behind it has rewritten the block: another stroke altogether
    far = np.array([[0, 0, 0], [S - 1, 0, 0], [0, S - 1, 0], [0, 0, S - 1]], np.uint32)
    edit = [("strokeAtHits", "devB", dict(stroke, then=("setVoxels", far)))]
    assert visible(edit, "links") and not visible([("strokeAtHits", "host", dict(stroke, then=None))], "links")
    good, bad = seen(edit, None)[0][1], seen(edit, "links")[0][1]
    assert (bad & (1 - good)).any()                                       # the first centres, rewritten, were never dug
    # the offsets block of the lists and the surface calls.  A count behind an extraction that did not wait: the extraction
    # emits by the count's offsets -- the step's own records differ; only the surfaceCount, which writes six slots that no
    # list reads, cannot show
    def lists(form, op, box, capacity=300, neighbours=False, first=0, **more):
        return ("voxels", form, dict(op=op, box=box, closed=True, neighbours=neighbours, first=first, capacity=capacity, skew=0, shift=1, **more))
    # (32^3 is four workgroups of x: the first window spans the end of the first, the second lies in one the count left empty)
    for step in (lists("devA", P.voxels_model.ALL, None, first=int(start[:8].sum()) - 150, order="extract_first"),
                 ("surface", "devB", dict(closed=True, first=0, capacity=300, order="voxels_behind", behind=dict(op=1, box=[9, 1, 1, 31, 31, 17], closed=True)))):
        good, bad = seen([step], None)[0][0], seen([step], "unordered")[0][0]
        assert good[0] == bad[0] and good[2] == bad[2] and good[1].shape == bad[1].shape and not np.array_equal(good[1], bad[1]), step[:2]
    assert not visible([lists("devA", P.voxels_model.ALL, None, order="count_first")], "unordered")
    assert not visible([lists("devA", P.voxels_model.ALL, None, order="surface_behind")], "unordered")
    # a host window sized by the total the block still held: a list with a large total, then one of a small box
    pair = [lists("host", P.voxels_model.ALL, None), lists("host", P.voxels_model.SURFACE, [3, 5, 3, 6, 8, 5], neighbours=True)]
    good, bad = seen(pair, None), seen(pair, "totals")
    assert P.same_value(good[0], bad[0]) and good[1][0][0] == bad[1][0][0] < 300
    assert len(bad[1][0][1]) == 300 > len(good[1][0][1]) and bad[1][2] - good[1][2] == 16 * 300 - 12 * 300       # and the staging block with it
    assert not visible(pair[:1], "totals") and not visible([pair[1], pair[1]], "totals")


def test_scratch_sizes_restate_the_per_family_tests():
    # tests/test_gpu_volume_surface.py: offsets_bytes; test_gpu_volume_rects.py: block_bytes and :313; test_gpu_volume_pack.py:48
    assert P.surface_bytes(6) == 8 * (8 ** 6 // 32 // 256 + 7) and P.rects_bytes(6) == 8 * (192 + 7) + 8 * 64 * 64 * 2
    assert P.pack_bytes(5) == 8 * (pack_model.Shape(5).NT + 1) + 64 and P.marks_bytes(10) == 1 << 27
    assert P.flood_bytes(5) == 4 * (3 + 8) and P.flood_bytes(6) == 4 * (24 + 8)
    m = P.Mirror(5)
    m.apply(("setVoxels", "host", dict(items=np.zeros((10, 3), np.uint32), solid=True)))
    m.apply(("getVoxels", "host", dict(items=np.zeros((3, 3), np.uint32))))
    m.apply(("surface", "devA", dict(closed=True, first=0, capacity=5)))
    assert m.scratch_bytes() == 120 + P.surface_bytes(5)
    m.apply(("cloneSecond", "host", {}))
    assert m.scratch_bytes("w") == 0
    # tests/test_gpu_stroke.py and test_gpu_volume_raster.py:154-166 (32 and 36 bytes an item), test_gpu_volume_columns.py:75, 183
    # (the records and the maps of the column calls: a block of the call's own, the volume's scratch does not move)
    m = P.Mirror(5)
    m.apply(("columnProfile", "host", dict(direction=2, rect=[0, 0, 3, 5])))
    m.apply(("fillColumns", "host", dict(axis=1, rect=[0, 0, 3, 5], op=P.OR, lo=np.zeros((3, 5), np.int32), hi=np.ones((3, 5), np.int32), maps=2)))
    assert m.scratch_bytes() == 0
    m.apply(("fillCapsules", "host", dict(items=np.zeros((10, 8), np.int32), solid=True)))
    m.apply(("columnProfile", "host", dict(direction=2, rect=[0, 0, 3, 5])))
    assert m.scratch_bytes() == 320
    m.apply(("rasterMesh", "host", dict(items=np.zeros((9, 9), np.int32), op=P.THIN, solid=True)))
    assert m.scratch_bytes() == 324
    m.apply(("fillCapsules", "devA", dict(items=np.zeros((99, 8), np.int32), solid=True)))
    m.apply(("rasterMesh", "dev0", dict(items=np.zeros((99, 9), np.int32), op=P.THIN, solid=True)))
    m.apply(("selectColumnsDst", "devA", dict(direction=0, lo=0, hi=1, of=1, op=P.OR)))
    assert m.scratch_bytes() == 324 and m.scratch_bytes("w") == 0
    hits = P.hits_of(np.zeros((21, 3), np.int64), 32)
    m.apply(("strokeAtHits", "devB", dict(hits=hits, radius=1, max_gap=0, solid=True, then=None)))
    assert m.scratch_bytes() == 16 * 21
    m.apply(("strokeAtHits", "host", dict(hits=hits, radius=1, max_gap=0, solid=True, then=None)))
    assert m.scratch_bytes() == 64 * 21
    # tests/test_gpu_volume_voxels.py: offsets_bytes (the surface calls' block, counted once) and :250 (record * window, bounded by
    # 2^20 records); a device-form list and the list into w stage nothing, an empty window reserves nothing
    m = P.Mirror(5)
    m.s["v"] = field(32, 5)
    T = int(m.s["v"].sum())
    for form, a in (("devA", dict(first=0, capacity=T)), ("host", dict(first=T, capacity=9)), ("host", dict(first=T - 7, capacity=9)), ("host", dict(first=0, capacity=5))):
        m.apply(("voxels", form, dict(a, op=0, box=None, closed=True, neighbours=form == "host", skew=0, order="count_first", shift=1)))
        assert m.scratch_bytes() == P.surface_bytes(5) + (16 * 7 if a["first"] == T - 7 or a["capacity"] == 5 else 0)
    m.apply(("listToSecond", "devB", dict(which=0, box=None, closed=True, solid=True, n=T)))
    m.apply(("surface", "host", dict(closed=True, first=0, capacity=0)))
    assert m.scratch_bytes() == P.surface_bytes(5) + 16 * 7 and m.scratch_bytes("w") == 0
    assert P.surface_bytes(5) == 8 * (4 + 7) and P.window_of(3, 1 << 40, 10) == 7 and P.window_of(11, 5, 10) == 0
