#!/usr/bin/env python3
"""Times the editable volume (vrc_volume_*) on the device, one JSON line.

For the 256^3, 512^3 and 1024^3 FastNoise terrain:
  from_scene_ms    wall time of vrc_volume_from_scene (allocation + rasterisation kernel, synchronous), median of 3
  set_voxels_ms    device time (events on the stream) of one vrc_volume_set_voxels batch of 1 / 1 000 / 10^6 random
                   voxels read from device memory, median of 5
  fill_box_64_ms   device time of one 64^3 box (vrc_volume_fill_boxes), median of 5
  commit_ms / build_volume_ms
                   vrc_volume_commit's build_ms against vrc_scene_build_volume's build_ms for the SAME occupancy in the
                   same process, alternating A B A B, `--pairs` pairs after one warm-up pair: medians, the baseline's
                   own min / max over its repetitions, and whether the commit's median lies within that spread
                   (commit_within_baseline_spread: commit median <= baseline max).
With --brushes (written to profiles/edit/bench_brushes.json by whoever runs it), the brushes, copies and queries instead,
at 512^3 and 1024^3, device memory, device time by events, one warm-up, A B A B in one process, `--pairs` pairs, median
and range:
  sphere_r{4,32,128}   one vrc_volume_fill_spheres sphere against vrc_volume_fill_boxes on that sphere's bounding box
  spheres_10k_r3       10^4 spheres of radius 3 in one batch
  spray_10k            cast 10^4 rays + brush at hits (radius 3) + commit on one stream, against the host round trip
                       (cast to host memory, vrc_hit_to_voxel per record, vrc_volume_set_voxels of the enumerated voxels,
                       commit); both end-to-end wall times
  copy_64              a 64^3 region copy at an aligned and at an odd offset
  clone                a whole-volume clone (wall time) and the fraction of HBM speed its bytes moved at
  get_voxels_1m, count_boxes_1k_16
With --flood (written to profiles/edit/bench_flood.json by whoever runs it), vrc_volume_flood at 512^3, device time by
events around the synchronous call, one warm-up, A B A B in one process against B = reading region and medium once (two
vrc_volume_solid_count calls, 32 MiB), `--pairs` pairs, median and range, with the sweeps issued and
read_once x sweeps as the floor a flood without frontier tracking could not beat:
  terrain_from_bottom      the FastNoise terrain's solid voxels from the slab its columns stand on
  dug_terrain_from_bottom  the same after 400 sphere digs of radius 12 at ray hits
  air_from_top             the EMPTY flood of the air above the dug terrain from the slab y = S - 1
  serpentine               the worst case: a one-voxel path of 1024 lines through every tile, from its first voxel
  host_round_trip          what the flood replaces, on the dug terrain: vrc_volume_download, a labelling pass in numpy
                           (tests/flood_model.py), upload of the result as y runs through vrc_volume_fill_boxes; wall times
With --voxelize (written to profiles/edit/bench_voxelize.json by whoever runs it), vrc_volume_xor_mesh at 512^3, triangles in
device memory, device time by events, one warm-up, A B A B in one process against B = one read of a field of the
occupancy's size (vrc_volume_solid_count, 16 MiB); the floor of the call is three such passes (read the marks, read and
write the occupancy) and is reported as floor_ms = 3 x read_once; `--pairs` pairs (one more if even, so that every mesh is XORed an even number of
times and the volume is empty again), median and range:
  icosphere_20k        an icosphere of 20 480 triangles, radius 200 voxels
  icosphere_1m         the same sphere as 1 310 720 triangles (three more subdivisions)
  spanning_box         one box mesh spanning the volume: 12 triangles of 2^18 columns each
  icospheres_4096      4 096 icospheres of 80 triangles, radius 6, at random places, in one call
  host_round_trip      what the call replaces, for icosphere_20k and spanning_box: the numpy model on the host
                       (tests/voxelize_model.py), then the upload of its result as z runs through vrc_volume_fill_boxes;
                       wall times
  first_call           wall time of the first call on a fresh volume (it allocates and zeroes the mark field) and of the second
With --surface (written to profiles/edit/bench_surface.json by whoever runs it), the surface extraction at 512^3, output in
device memory, device time by events on the NULL stream, one warm-up, A B A B in one process against B =
vrc_volume_solid_count on the same volume (it reads the same words once), `--pairs` pairs, median and range, the ratio to B:
  terrain              the FastNoise terrain
  dug_terrain          the same after the flood mode's digs (400 spheres of radius 12 at ray hits)
  stamped_noise        the dug terrain with a random 128^3 field of density 0.5 stamped in
  per volume: count (vrc_volume_surface_count), faces / triangles (vrc_volume_extract_surface of ALL faces, closed), the
  number of faces and the bytes written
With --rects (printed and written to profiles/edit/bench_rects.json), the merged-rectangle extraction at 512^3 next to the
surface extraction on the same volumes in the same run, output in device memory, device time by events on the NULL stream,
one warm-up, A B A B in one process with A the rectangle call and B the surface call it replaces, `--pairs` pairs, median and
range:
  terrain              the FastNoise terrain
  dense_noise          a random field of density 0.5 in the 128^3 corner box [0, 128)^3 of an otherwise empty volume
  per volume: faces T and rectangles R with T / R, count (vrc_rect_count next to vrc_volume_surface_count), records
  and triangles (vrc_extract_rects of ALL rectangles next to vrc_volume_extract_surface of ALL faces, closed) and the
  bytes each writes
With --components (printed and written to profiles/edit/bench_components.json), the connected-component labelling at 512^3,
device time by events on the NULL stream around the synchronous calls, one warm-up, `--pairs` repetitions, median and range:
  terrain / dug_terrain / dug_terrain_26 / air
                       the FastNoise terrain, the same after the flood mode's digs (400 spheres of radius 12 at ray hits)
                       under 6 and 26, and the air above it (through the empty voxels).  Per case: label (the whole
                       vrc_volume_label_components call), records (all of them to host memory, wall time), select_one (the
                       largest piece into a fresh volume, keep in device memory), select_all, remove_small (wall time of
                       VoxelVolume.removeSmallPieces(8) on a clone), the number of pieces and the largest
  scale                on the dug terrain, in the same run: fill_ids = a plain device fill of an array of the id array's size
                       (4 bytes per voxel; the labelling is expected to cost a small number of such passes), solid_count,
                       one full vrc_volume_flood from the bottom slab, and flood_per_piece = what the labelling replaces:
                       one vrc_volume_flood from each record's `first` for at most the 16 largest pieces, and that mean
                       times the number of pieces (EXTRAPOLATED, labelled so)
With --distance (printed and written to profiles/edit/bench_distance.json), the exact distance field at 512^3, device time
by events on the NULL stream around the calls, one warm-up, `--pairs` repetitions, median and range, for to = SOLID and EMPTY:
  terrain / corner_voxel / empty
                       the FastNoise terrain, a volume with one solid voxel in a corner (the long-parabola worst case: for
                       to = SOLID one parabola spans every line) and an empty volume (to = SOLID: no feature at all,
                       to = EMPTY: every voxel one).  Per case: field (the whole vrc_volume_distance_field call), select
                       (vrc_distance_select of [0, 16] into a fresh volume), dilate_4 (VoxelVolume.dilate(4) on a clone, end
                       to end, wall time), the stats, and field_over_copy
  copy_field           the yardstick, in the same run: a device-to-device copy of 4 S^3 bytes (one read and one write of the
                       field; the transform reads and writes it twice after writing it once)
  worst_over_terrain   field time of corner_voxel over field time of terrain, per `to`: the per-line bound in practice
With --stamp (printed and written to profiles/edit/bench_stamp.json), the affine stamp at 512^3 from the FastNoise terrain
into a second volume, device time by events on the NULL stream, one warm-up, A B A B in one process, `--pairs` pairs, median
and range:
  identity             A = vrc_volume_copy_region of the whole volume, B = vrc_volume_stamp_affine with the identity map over
                       the same box (the same work without and with the map: the yardstick), the two results asserted equal,
                       and stamp_over_copy
  quarter_turn         q = (p_y, S-1-p_x, p_z), next to the same copy
  turn_30_30           a 30-degree turn about two axes at scale 1 about the centre (vrc_affine_place's map and box)
  clipboard_64_x2      a 64^3 clipboard cut from the terrain's surface, stamped at scale 2 with the same turn into the world
                       with the box from vrc_affine_place, next to a 128^3 region copy
  per case the solid voxels of the result
With --travel (printed and written to profiles/edit/bench_travel.json), the travel-distance field at 512^3 on the FastNoise
terrain, device time by events on the NULL stream around the synchronous calls, one warm-up, `--pairs` repetitions, median and
range, for 6 and 26 neighbours:
  air_from_one_seed    through the empty voxels from the highest empty voxel of the centre column
  solid_from_the_floor through the solid voxels from the floor layer, the slab y = S / 2 + 1 the terrain's columns stand on
  per case: travel (the whole vrc_travel_field call) with seeds, reached, max_steps and the sweeps issued; flood
  (vrc_volume_flood from the same seeds on the same medium, in the same run: the support of the same field) with its sweeps
  and reached, which equals the field's; and travel_over_flood
With --fall (printed and written to profiles/edit/bench_fall.json), falling pieces at 512^3 on the FastNoise terrain: a band of
four layers is carved out of the terrain 24 voxels above the slab its columns stand on and one of three layers 44 voxels
above it, and everything above the lower band is cut by planes two voxels thick every 32 voxels along x and z, so that it
hangs loose in a few hundred blocks, those above the upper band over those below it; keepConnected from the slab splits the
supported part from the debris.  Device time by events on
the NULL stream, one warm-up, `--pairs` repetitions, median and range:
  label      vrc_volume_label_components of the debris (the comparison figure: a fall is a few more passes over its id array)
  fall       vrc_fall_drops towards -y over the supported part, offsets in device memory, with rounds, pieces, moved pieces
             and voxels and the largest drop
  place      vrc_fall_place of every piece into a copy of the supported part (OR), offsets in device memory
  select     vrc_labels_select of every piece of the same labels into a volume (OR)
  fall_round_over_label = fall / rounds / label
With --fracture (printed and written to profiles/edit/bench_fracture.json), Voronoi fracture at 512^3 on the FastNoise terrain,
sites in device memory, device time by events on the NULL stream around the synchronous calls, one warm-up pair, A B A B in one
process, `--pairs` pairs, median and range; A = vrc_fracture_label, B = vrc_volume_distance_field followed by
vrc_volume_label_components of the same medium (the yardstick: the same traffic plus the index):
  impact_64_sites_radius_48   64 sites within 48 voxels of a surface point (scenes.scatter_sites), max_distance 48
  whole_volume_4096_sites     4096 sites over the whole volume, no cut-off
  fracture_over_distance_plus_label = A / B; the passes are not timed apart
With --rigid (printed and written to profiles/edit/bench_rigid.json), the pieces as rigid bodies on the --fall scene (the same
terrain, bands and cuts: a few hundred loose blocks), device time by events on the NULL stream, one warm-up, `--pairs`
repetitions, median and range, everything in device memory:
  moments          vrc_rigid_moments of all pieces              next to  select: vrc_labels_select of all pieces (one pass over
                                                                         the same id array, no sums)
  place_translate  vrc_rigid_place_affine with pure-translation maps (the fall's offsets; boxes = the record boxes moved by
                   them)                                        next to  fall_place: vrc_fall_place with the same offsets; the
                                                                         two results are compared voxel for voxel
  place_turn       vrc_rigid_place_affine with every piece turned 30 degrees about x, then y, about its own centre of mass
                   (maps and boxes from VoxelLabels.poses)
With --contacts (printed and written to profiles/edit/bench_contacts.json), the contact test of posed pieces on the same scene,
timed the same way, everything in device memory; each contact call next to vrc_rigid_place_affine with the same maps and boxes
in the same run (the contact time includes the zeroing of the records; the passes of a call are not timed apart):
  contacts_translate  vrc_rigid_contacts with the fall's translation maps and the moved record boxes against the supported
                      part                                      next to  place_translate
  contacts_turn       the same with every piece turned 30 degrees about x, then y, about its own centre of mass
                                                                next to  place_turn
  contacts_*_full     the two again with world = the whole medium (supported part and debris): most gathered words are
                      non-zero in the world
With --pair-contacts (printed and written to profiles/edit/bench_pair_contacts.json), posed pieces against each other on the same
scene with the turned poses of --contacts, timed the same way, everything in device memory:
  box_pairs_count_and_list  vrc_rigid_box_pair_count + vrc_rigid_box_pairs of all candidate pairs (both synchronous; the
                            allocation of their scratch is inside the events)
  pair_contacts             vrc_rigid_pair_contacts over all candidate pairs, the zeroing of the records included; how many
                            pairs overlap and how many touch
  yardstick_per_pair        the documented workaround on a sample of at most 64 of the pairs, evenly spaced in the list
                            (yardstick_sample_pairs): the scratch volume cleared, vrc_rigid_place_affine of b alone into it,
                            vrc_rigid_contacts of a alone against it; yardstick_scaled = its median times the number of pairs
Measured on an MI355X at 512^3: 404 pieces, 3688 candidate pairs listed in 0.33 ms, their records in 0.81 ms (652 pairs
overlap, 798 touch), next to 0.098 ms per pair of the workaround on 64 pairs, 360 ms scaled, 445 times.  Not timed apart: the
zeroing, the two gathers and the reduction of the pair kernel; the count, scan and emit of the broad phase; the three steps
of the workaround.
With --clearance (printed and written to profiles/edit/bench_clearance.json), a field read at the voxels of posed pieces on the
same scene, everything in device memory, A B A B in one run: each clearance call over the Euclidean field of the supported part
next to vrc_rigid_contacts against the supported part with the same maps and boxes -- the same gather, reading at most 7 words
where the clearance reads up to 32 values (the clearance time includes its two one-thread-per-record kernels, the contact time
the zeroing of the records; the passes of a call are not timed apart):
  clearance_translate  vrc_rigid_clearance with the fall's translation maps and the moved record boxes
                                                                next to  contacts_translate
  clearance_turn       the same with every piece turned 30 degrees about x, then y, about its own centre of mass
                                                                next to  contacts_turn
With --delta (printed and written to profiles/edit/bench_delta.json), the deltas at 512^3 on the FastNoise terrain, device
time by events on the NULL stream, one warm-up pair, A B A B in one process, `--pairs` pairs, median and range.  Per case --
  sphere_dig_r8      the terrain before and after a radius-8 sphere dug at its surface
  drop_loose         the fall benchmark's scene (--fall) before and after VoxelVolume.dropLoose
  terrain_vs_empty   the terrain against an empty volume: about half of all words differ
-- diff_ms (vrc_delta_diff, its scratch allocation, the read-back of the count and the allocation of the records inside the
events; the object is destroyed outside them) next to clone_ms (vrc_volume_clone, the undo snapshot it replaces, timed the same
way), then apply_ms (vrc_delta_apply onto the `before` volume, twice per sample so that the volume is left as it was, halved)
next to copy_ms (a device-to-device copy of one occupancy: the floor for scale), and the records, their bytes and the bytes
over the occupancy a clone holds.
Measured on an MI355X at 512^3: the diff 0.072 / 0.113 / 0.151 ms for 70 / 74877 / 300737 records next to 0.037 ms for the clone,
the apply 0.009 ms in all three next to 0.008 ms for the copy.  Not timed apart: the allocations, the read-back and the three
kernels of the diff.
With --cells (printed and written to profiles/edit/bench_cells.json), the cell calls at 512^3, device time by events on the
NULL stream, a sample = 20 calls in a row between two events, divided; one warm-up pair, A B A B in one process, `--pairs` pairs,
median and range, on two inputs -- the FastNoise terrain and a fillRandom of density 0.5 -- each entry next to one of the library's existing read-once / write-once passes over the same
16 MiB, timed in the same pair:
  step_6 / step_26                   vrc_cells_step into a second volume, no counter       next to  copy_region (whole volume, REPLACE)
  step_6_changed / step_26_changed   the same with `changed` in device memory              next to  clone (vrc_volume_clone, closed outside the events)
  fill_random                        vrc_cells_fill_random of the whole volume, REPLACE    next to  copy_region
and step_over_copy, the ratio of the medians.  The smoothing rule (majority of 27) and, with six neighbours, survive = 1 .. 6.
With --pack (printed and written to profiles/edit/bench_pack.json), the sparse tile stream at 512^3, device time by events on
the NULL stream, one warm-up round, median of `--pairs` rounds, every call of a round in the same process, on two inputs -- the
FastNoise terrain and a fillRandom of density 0.5, the format's worst case.  Per input the stream's bytes, M and P, and
  size_ms      vrc_pack_volume without a buffer: the count and scan passes and the read-back of the totals
  pack_ms      vrc_pack_volume into device memory: the same, then the emit
  unpack_ms    vrc_unpack_volume from device memory: the header copy, the checks, the read-back of the totals, the write
  clone_ms     vrc_volume_clone (closed outside the events)
  download_ms  vrc_volume_download, one byte per voxel to the host
With --columns (printed and written to profiles/edit/bench_columns.json), the column calls at 512^3, device time by events on
the NULL stream, a sample = 20 calls in a row between two events, divided; one warm-up pair, A B A B in one process, `--pairs`
pairs, median and range, on two inputs -- the FastNoise terrain and a fillRandom of density 0.5 -- every list in device memory,
each entry next to an existing pass over the same 16 MiB, timed in the same pair:
  profile_x / _y / _z    vrc_columns_profile of the whole face (4 MiB of records)          next to  solid_count and clone
  raise_terrain          vrc_columns_fill along y from the 512^2 FastNoise heights, REPLACE  next to  fill_boxes (one box, the whole volume)
  select_x / _y / _z     vrc_columns_select (0, 1, SOLID) into a second volume               next to  cells_step with 6 neighbours
and the ratios of the medians.
No ratio is promised and no threshold is applied; the numbers are reported."""
import argparse
import collections
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(values, digits=5):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def event_ms(fn):
    """(device ms between two events on the NULL stream around fn(), what fn returned)"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def device_ms(fn, repeats=5):
    return statistics.median([event_ms(fn)[0] for _ in range(repeats + 1)][1:])          # the first run warms up


def timed(fn, repeats, digits=4, before=None, after=None):
    """One call over `repeats` samples after one warm-up: returns (stat, the last result).  The previous result is closed, if
    it can be, before the next pair of events.  With `before`, fn takes what before() made outside the events, and
    after(result, that) -- outside them too -- gives what is kept as the result."""
    out, last = [], None
    for i in range(repeats + 1):
        if last is not None and hasattr(last, "close"):
            last.close()
        arg = before() if before else None
        ms, last = event_ms((lambda: fn(arg)) if before else fn)
        if i:
            out.append(ms)
        if after:
            last = after(last, arg)
    return stat(out, digits), last


def timed_ab(fns, pairs, calls=1, digits=5):
    """A B (C ...) A B (C ...) after one warm-up round: a sample is `calls` calls in a row between two events, divided.  What a
    call returns is closed, if it can be, after the events.  One stat per function."""
    out = [[] for _ in fns]
    for i in range(pairs + 1):
        for k, fn in enumerate(fns):
            ms, made = event_ms(lambda: [fn() for _ in range(calls)])
            for thing in made:
                if hasattr(thing, "close"):
                    thing.close()
            if i:
                out[k].append(ms / calls)
    return [stat(o, digits) for o in out]


def ab_device_ms(fa, fb, pairs):
    """A B A B: device time of each by events on the NULL stream, one warm-up pair first"""
    return timed_ab((fa, fb), pairs)


def ab_wall_ms(fa, fb, pairs):
    import torch
    out = ([], [])
    for i in range(pairs + 1):
        for k, fn in enumerate((fa, fb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i:
                out[k].append((time.perf_counter() - t0) * 1e3)
    return stat(out[0], 3), stat(out[1], 3)


HBM_BYTES_PER_S = 8.0e12     # MI355X peak


def fall_cuts(S):
    """(the boxes the fall benchmark clears from the terrain, the slab its columns stand on): a band of four layers 24 voxels
    above the slab (the first box), one of three layers 44 above it, and from the lower band up planes two voxels thick every
    32 voxels along x and z"""
    floor_y = S // 2 + 1
    cuts = [[0, floor_y + 24, 0, S, floor_y + 28, S], [0, floor_y + 44, 0, S, floor_y + 47, S]]
    cuts += [[c, floor_y + 24, 0, c + 2, S, S] for c in range(30, S, 32)] + [[0, floor_y + 24, c, S, S, c + 2] for c in range(30, S, 32)]
    return cuts, [[0, floor_y, 0, S, floor_y + 1, S]]


def fall_scene(vrc, depth, label=True, whole=False):
    """The fall benchmark's scene (the module's text, --fall): the FastNoise terrain with fall_cuts cleared, split by
    keepConnected from the slab.  Returns (scene, world = the supported part, debris, the debris' labels or None without
    `label`, and with `whole` a clone of the medium taken before the split, else None)."""
    cuts, slab = fall_cuts(1 << depth)
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    world = vrc.VoxelVolume.fromScene(scene)
    world.fillBoxes(cuts, False)
    full = world.clone() if whole else None
    debris = world.keepConnected(slab, 6)
    return scene, world, debris, debris.labelComponents(6) if label else None, full


def turn_30_30():
    """a rotation by 30 degrees about x, then about y, in vrc_make_rotation's layout (columns)"""
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.ascontiguousarray((ry @ rx).T, np.float32).reshape(9)


def turn_poses(labels):
    """(maps, boxes) of every piece turned by turn_30_30 about its own centre of mass"""
    return labels.poses(turn_30_30(), labels.massProperties()[1])


def translate_poses(labels, records, offsets, S):
    """(maps, boxes) of every piece moved by its row of `offsets` (the fall's): pure-translation maps, the record boxes moved"""
    from cpuvoxelraycaster_amd import capi
    maps = np.zeros(labels.count, capi.AFFINE_DTYPE)
    maps["m"][:] = [65536, 0, 0, 0, 65536, 0, 0, 0, 65536]
    maps["t"][:] = -(offsets.astype(np.int64) << 17)
    boxes = np.concatenate([np.clip(records["lo"].astype(np.int64) + offsets, 0, S), np.clip(records["hi"].astype(np.int64) + offsets, 0, S)], axis=1).astype(np.uint32)
    return maps, boxes


def box_words(boxes):
    """the (piece, destination word) work items of the placement: vrc_box_words.h's count over the non-empty boxes"""
    return int(sum(((int(b[3]) - 1) // 2 - int(b[0]) // 2 + 1) * ((int(b[4]) - 1) // 2 - int(b[1]) // 2 + 1) * ((((int(b[5]) - 1) // 2 - int(b[2]) // 2) + 3) // 4 + 1)
                   for b in boxes if all(b[a] < b[a + 3] for a in range(3))))


def on_device(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).cuda()


def bench_brushes(vrc, depth, pairs):
    import torch
    S = 1 << depth
    rng = np.random.default_rng(depth)
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    res = {"size": S, "pairs": pairs}
    flip = [False]
    m = S // 2

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()

    for r in (4, 32, 128):
        sphere = dev(np.array([(m, m, m, r)], np.int32))
        box = dev(np.array([(m - r, m - r, m - r, m + r + 1, m + r + 1, m + r + 1)], np.uint32))

        def fa():
            flip[0] = not flip[0]
            volume.fillSpheresDevice(1, sphere.data_ptr(), flip[0], None)

        def fb():
            volume.fillBoxesDevice(1, box.data_ptr(), flip[0], None)
        a, b = ab_device_ms(fa, fb, pairs)
        res[f"sphere_r{r}"] = {"sphere_ms": a, "bounding_box_ms": b, "sphere_not_slower": bool(a["median"] <= b["median"])}
    spheres = dev(np.concatenate([rng.integers(0, S, (10000, 3)), np.full((10000, 1), 3)], axis=1).astype(np.int32))
    res["spheres_10k_r3_ms"] = ab_device_ms(lambda: volume.fillSpheresDevice(10000, spheres.data_ptr(), True, None),
                                            lambda: volume.fillSpheresDevice(10000, spheres.data_ptr(), False, None), pairs)[0]
    volume.close()

    # spray: 10^4 camera rays, dig radius 3 at every hit, commit -- device path against today's host round trip
    volume = vrc.VoxelVolume.fromScene(scene)
    other = vrc.VoxelVolume.fromScene(scene)
    cam = np.array(vrc.reference_camera_position(depth), np.float32) / np.float32(S) + np.float32(1.0)
    d = rng.normal(size=(10000, 3)).astype(np.float32) * np.float32(0.3) + np.array([0.0, 0.5, 0.8], np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    org = np.tile(cam, (10000, 1)).astype(np.float32)
    t_org, t_dir, t_hits = dev(org), dev(d), torch.zeros(10000 * 12, dtype=torch.int32).cuda()
    g = np.mgrid[-3:4, -3:4, -3:4].reshape(3, -1).T
    ball = g[(g * g).sum(1) <= 9]
    L = vrc.capi.load()
    import ctypes as C
    stream = C.c_void_p()
    vrc.capi.check(L.vrc_stream_create(0, C.byref(stream)))
    counts = {}

    def device_path():
        scene.castRaysDevice(10000, t_org.data_ptr(), t_dir.data_ptr(), t_hits.data_ptr(), stream=stream)
        volume.fillSpheresAtHitsDevice(10000, t_hits.data_ptr(), 3, False, stream)
        volume.commit().close()

    def host_path():
        hits = scene.castRays(org, d)
        xyz = []
        for h in hits[(hits["hit"] & 0xff) == 1]:
            xyz.append(np.array(vrc.hit_to_voxel(depth, h)[0]) + ball)
        if xyz:
            xyz = np.concatenate(xyz)
            xyz = xyz[np.all((xyz >= 0) & (xyz < S), axis=1)]
            other.setVoxels(xyz.astype(np.uint32), False)
            counts["voxels_sent"] = int(len(xyz))
        other.commit().close()
    a, b = ab_wall_ms(device_path, host_path, pairs)
    assert volume.solidCount() == other.solidCount()
    res["spray_10k"] = {"device_path_wall_ms": a, "host_round_trip_wall_ms": b, **counts}
    L.vrc_stream_synchronize(0, stream)
    L.vrc_stream_destroy(0, stream)
    other.close()

    # copies
    clip = vrc.VoxelVolume(6)
    clip.fillSpheres([(32, 32, 32, 30)], True)
    a, b = ab_device_ms(lambda: volume.copyRegion(clip, [0, 0, 0], [64, 64, 64], [m, m, m], 0, None),
                        lambda: volume.copyRegion(clip, [0, 0, 0], [64, 64, 64], [m + 1, m + 1, m + 3], 0, None), pairs)
    res["copy_64_ms"] = {"aligned": a, "odd_offset": b}
    walls = []
    for i in range(pairs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = volume.clone()
        if i:
            walls.append((time.perf_counter() - t0) * 1e3)
        c.close()
    moved = 2 * (S ** 3 // 8)                               # read + write of the brick bytes
    res["clone"] = {"wall_ms": stat(walls, 3), "bytes_moved": moved,
                    "fraction_of_hbm_peak": round(moved / HBM_BYTES_PER_S / (statistics.median(walls) * 1e-3), 4)}

    # queries
    xyz = dev(rng.integers(0, S, (1000000, 3)).astype(np.uint32))
    out = torch.zeros(1000000, dtype=torch.uint8).cuda()
    lo = rng.integers(0, S - 16, (1000, 3))
    boxes = dev(np.concatenate([lo, lo + 16], axis=1).astype(np.uint32))
    cnt = torch.zeros(1000, dtype=torch.int64).cuda()
    a, b = ab_device_ms(lambda: volume.getVoxelsDevice(1000000, xyz.data_ptr(), out.data_ptr(), None),
                        lambda: volume.countBoxesDevice(1000, boxes.data_ptr(), cnt.data_ptr(), None), pairs)
    res["get_voxels_1m_ms"], res["count_boxes_1k_16_ms"] = a, b
    volume.close()
    clip.close()
    scene.close()
    return res


def bench_flood(vrc, depth, pairs):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import flood_model
    S = 1 << depth
    rng = np.random.default_rng(depth)
    res = {"size": S, "pairs": pairs, "read_once_bytes": 2 * (S ** 3 // 8)}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    region = vrc.VoxelVolume(depth)
    whole = np.array([[0, 0, 0, S, S, S]], np.uint32)
    bottom = np.array([[0, S // 2 + 1, 0, S, S // 2 + 2, S]], np.uint32)
    top = np.array([[0, S - 1, 0, S, S, S]], np.uint32)

    def case(medium, seed, connectivity, through_empty, seed_is_voxels=False):
        stats = []

        def fa():
            region.fillBoxes(whole, False)
            (region.setVoxels if seed_is_voxels else region.fillBoxes)(seed)
            ms, st = event_ms(lambda: region.flood(medium, connectivity, through_empty))
            assert st.converged == 1
            stats.append((ms, st.sweeps, st.reached))

        def fb():
            region.solidCount()
            medium.solidCount()
        flood_ms, reads = [], []
        for i in range(pairs + 1):
            fa()
            ms, _ = event_ms(fb)
            if i:
                flood_ms.append(stats[-1][0])
                reads.append(ms)
        sweeps = stats[-1][1]
        assert all(s[2] == stats[-1][2] for s in stats)
        floor = statistics.median(reads) * sweeps
        return {"connectivity": connectivity, "through_empty": through_empty, "flood_ms": stat(flood_ms, 4), "sweeps": sweeps,
                "sweeps_range": [min(s[1] for s in stats), max(s[1] for s in stats)], "reached": stats[-1][2],
                "read_once_ms": stat(reads, 4), "read_once_x_sweeps_ms": round(floor, 4),
                "flood_over_floor": round(statistics.median(flood_ms) / floor, 4)}

    res["terrain_from_bottom"] = case(terrain, bottom, 6, False)
    cam = np.array(vrc.reference_camera_position(depth), np.float32) / np.float32(S) + np.float32(1.0)
    d = rng.normal(size=(400, 3)).astype(np.float32) * np.float32(0.3) + np.array([0.0, 0.5, 0.8], np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    hits = scene.castRays(np.tile(cam, (400, 1)).astype(np.float32), d)
    terrain.fillSpheresAtHits(hits, 12, False)
    res["digs"] = {"rays": 400, "unit_hits": int(((hits["hit"] & 0xff) == 1).sum()), "radius": 12}
    res["dug_terrain_from_bottom"] = case(terrain, bottom, 6, False)
    res["dug_terrain_from_bottom_26"] = case(terrain, bottom, 26, False)
    res["air_from_top"] = case(terrain, top, 6, True)

    # what the flood replaces: download, label on the host, upload the result as runs along y
    walls = {}
    t0 = time.perf_counter()
    dug = terrain.download()
    walls["download_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    seeds = np.zeros_like(dug)
    seeds[:, S // 2 + 1, :] = 1
    want = flood_model.flood(dug, seeds, 6)
    walls["host_labelling_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    edge = np.diff(np.pad(want.astype(np.int8), ((0, 0), (1, 1), (0, 0))), axis=1)
    starts, ends = np.argwhere(edge == 1), np.argwhere(edge == -1)          # sorted by (x, y, z): re-sort by (x, z, y) to pair them
    starts = starts[np.lexsort((starts[:, 1], starts[:, 2], starts[:, 0]))]
    ends = ends[np.lexsort((ends[:, 1], ends[:, 2], ends[:, 0]))]
    boxes = np.stack([starts[:, 0], starts[:, 1], starts[:, 2], starts[:, 0] + 1, ends[:, 1], starts[:, 2] + 1], axis=1).astype(np.uint32)
    other = vrc.VoxelVolume(depth)
    other.fillBoxes(boxes)
    torch.cuda.synchronize()
    walls["upload_fill_boxes_ms"] = (time.perf_counter() - t0) * 1e3
    assert other.solidCount() == int(want.sum(dtype=np.int64)) == res["dug_terrain_from_bottom"]["reached"]
    other.close()
    res["host_round_trip"] = {k: round(v, 1) for k, v in walls.items()}
    res["host_round_trip"]["boxes_uploaded"] = int(len(boxes))
    res["host_round_trip"]["total_ms"] = round(sum(walls.values()), 1)
    del dug, seeds, want, edge

    path, start = flood_model.serpentine(S, 16)
    medium = vrc.VoxelVolume(depth)
    medium.setVoxels(np.argwhere(path))
    res["serpentine"] = case(medium, np.array([start], np.uint32), 6, False, seed_is_voxels=True)
    res["serpentine"]["path_voxels"] = int(path.sum())
    for v in (medium, region, terrain, scene):
        v.close()
    return res


def subdivided_icosphere(vrc, subdivisions):
    """scenes.icosphere beyond its three levels: every triangle split in four, new vertices pushed out to the unit sphere"""
    verts, faces = vrc.icosphere(min(subdivisions, 3))
    faces = faces.astype(np.int64)
    for _ in range(max(0, subdivisions - 3)):
        edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
        unique, inverse = np.unique(edges, axis=0, return_inverse=True)
        mid = verts[unique[:, 0]] + verts[unique[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inverse.reshape(3, -1) + len(verts)                  # midpoints of a-b, b-c, c-a per face
        a, b, c = faces.T
        faces = np.concatenate([np.stack(t, axis=1) for t in ((a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2]))])
        verts = np.concatenate([verts, mid])
    return verts, faces


def bench_voxelize(vrc, depth, pairs):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import voxelize_model
    S = 1 << depth
    rng = np.random.default_rng(depth)
    res = {"size": S, "pairs": pairs, "field_bytes": S ** 3 // 8}
    quantise = vrc.VoxelVolume.quantiseMesh

    def soup(verts, faces, scale, offset):
        return quantise(verts, scale, offset)[np.asarray(faces, np.int64)].reshape(-1, 9)

    m = S / 2
    meshes = {"icosphere_20k": soup(*subdivided_icosphere(vrc, 5), 200.0 * S / 512, (m + 0.3, m - 0.2, m + 0.1)),
              "icosphere_1m": soup(*subdivided_icosphere(vrc, 8), 200.0 * S / 512, (m + 0.3, m - 0.2, m + 0.1)),
              "spanning_box": soup(*vrc.box_mesh((0, 0, 0), (S, S, S)), 1.0, (0, 0, 0))}
    small_v, small_f = vrc.icosphere(1)
    meshes["icospheres_4096"] = np.concatenate([soup(small_v, small_f, 6.0, c) for c in rng.uniform(8, S - 8, (4096, 3))])

    # the first call allocates and zeroes the mark field
    fresh = vrc.VoxelVolume(depth)
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fresh.xorMesh(meshes["spanning_box"])
        walls.append(round((time.perf_counter() - t0) * 1e3, 3))
    res["first_call"] = {"first_wall_ms": walls[0], "second_wall_ms": walls[1]}
    fresh.close()

    # ab_device_ms calls the mesh once to warm up and once per timed pair: an odd number of pairs makes that an even number
    # of XORs, and the volume is empty again for the next mesh
    timed = pairs | 1
    res["pairs"] = timed
    volume = vrc.VoxelVolume(depth)
    for name, tris in meshes.items():
        t = torch.from_numpy(np.ascontiguousarray(tris, np.int32)).cuda()
        torch.cuda.synchronize()
        a, b = ab_device_ms(lambda: volume.xorMesh((len(tris), t.data_ptr()), device=True), lambda: volume.solidCount(), timed)
        res[name] = {"triangles": int(len(tris)), "xor_mesh_ms": a, "read_once_ms": b, "floor_ms": round(3 * b["median"], 5),
                     "over_floor": round(a["median"] / (3 * b["median"]), 3)}
        assert volume.solidCount() == 0, name
    volume.close()

    for name in ("icosphere_20k", "spanning_box"):
        walls = {}
        t0 = time.perf_counter()
        want = voxelize_model.xor_mesh(S, meshes[name])
        walls["host_model_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        edge = np.diff(np.pad(want.astype(np.int8), ((0, 0), (0, 0), (1, 1))), axis=2)
        starts, ends = np.argwhere(edge == 1), np.argwhere(edge == -1)      # both sorted by (x, y, z): they pair up in order
        boxes = np.concatenate([starts, ends + (1, 1, 0)], axis=1).astype(np.uint32)
        other = vrc.VoxelVolume(depth)
        other.fillBoxes(boxes)
        torch.cuda.synchronize()
        walls["upload_fill_boxes_ms"] = (time.perf_counter() - t0) * 1e3
        check = vrc.VoxelVolume(depth)
        check.xorMesh(meshes[name])
        assert other.solidCount() == check.solidCount() == int(want.sum(dtype=np.int64))
        other.close()
        check.close()
        res[name]["host_round_trip"] = {**{k: round(v, 1) for k, v in walls.items()}, "boxes_uploaded": int(len(boxes)),
                                        "total_ms": round(sum(walls.values()), 1), "solid_voxels": int(want.sum(dtype=np.int64))}
        del want, edge
    return res


def bench_surface(vrc, depth, pairs):
    import torch
    S = 1 << depth
    rng = np.random.default_rng(depth)
    res = {"size": S, "pairs": pairs, "read_once_bytes": S ** 3 // 8}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    volume = vrc.VoxelVolume.fromScene(scene)

    def case():
        counts = volume.surfaceCount()
        T = int(counts.sum())
        out = {"faces": T, "per_direction": [int(c) for c in counts], "solid": volume.solidCount()}
        count_ms, read_ms = ab_device_ms(volume.surfaceCount, volume.solidCount, pairs)
        out["count_ms"], out["read_once_ms"] = count_ms, read_ms
        out["count_over_read_once"] = round(count_ms["median"] / read_ms["median"], 3)
        for name, fmt, record in (("faces", vrc.capi.VRC_SURFACE_FACES, 16), ("triangles", vrc.capi.VRC_SURFACE_TRIANGLES, 72)):
            buf = torch.empty(max(T, 1) * record // 4, dtype=torch.int32, device="cuda")
            total = torch.zeros(1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ms, read_ms = ab_device_ms(lambda: volume.extractSurfaceDevice(fmt, 0, T, buf.data_ptr(), total.data_ptr()), volume.solidCount, pairs)
            assert int(total.item()) == T
            out[name + "_ms"], out[name + "_bytes"] = ms, T * record
            out[name + "_over_read_once"] = round(ms["median"] / read_ms["median"], 3)
            del buf
        return out

    res["terrain"] = case()
    cam = np.array(vrc.reference_camera_position(depth), np.float32) / np.float32(S) + np.float32(1.0)
    d = rng.normal(size=(400, 3)).astype(np.float32) * np.float32(0.3) + np.array([0.0, 0.5, 0.8], np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    hits = scene.castRays(np.tile(cam, (400, 1)).astype(np.float32), d)
    volume.fillSpheresAtHits(hits, 12, False)
    res["digs"] = {"rays": 400, "unit_hits": int(((hits["hit"] & 0xff) == 1).sum()), "radius": 12}
    res["dug_terrain"] = case()
    noise = vrc.VoxelVolume(7)
    noise.setVoxels(np.argwhere(rng.random((128, 128, 128)) < 0.5))
    volume.copyRegion(noise, (0, 0, 0), (128, 128, 128), (S // 2 - 64, S // 2, S // 2 - 64))
    res["stamped_noise"] = case()
    noise.close()
    volume.close()
    return res


def bench_rects(vrc, depth, pairs):
    import torch
    S = 1 << depth
    rng = np.random.default_rng(depth)
    res = {"size": S, "pairs": pairs}

    def case(volume):
        T, R = int(volume.surfaceCount().sum()), int(volume.rectCount().sum())
        out = {"faces": T, "rects": R, "faces_over_rects": round(T / max(R, 1), 3), "solid": volume.solidCount(),
               "rects_per_direction": [int(c) for c in volume.rectCount()]}
        out["rect_count_ms"], out["surface_count_ms"] = ab_device_ms(volume.rectCount, volume.surfaceCount, pairs)
        for name, fmt, record in (("records", vrc.capi.VRC_SURFACE_FACES, 16), ("triangles", vrc.capi.VRC_SURFACE_TRIANGLES, 72)):
            rects = torch.empty(max(R, 1) * record // 4, dtype=torch.int32, device="cuda")
            faces = torch.empty(max(T, 1) * record // 4, dtype=torch.int32, device="cuda")
            total = torch.zeros(2, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ms, surface_ms = ab_device_ms(lambda: volume.extractRectsDevice(fmt, 0, R, rects.data_ptr(), total.data_ptr()),
                                          lambda: volume.extractSurfaceDevice(fmt, 0, T, faces.data_ptr(), total.data_ptr() + 8), pairs)
            assert total.tolist() == [R, T]
            out["rect_" + name + "_ms"], out["surface_" + name + "_ms"] = ms, surface_ms
            out["rect_" + name + "_bytes"], out["surface_" + name + "_bytes"] = R * record, T * record
            del rects, faces
        return out

    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    volume = vrc.VoxelVolume.fromScene(scene)
    res["terrain"] = case(volume)
    volume.close()
    volume = vrc.VoxelVolume(depth)
    volume.setVoxels(np.argwhere(rng.random((128, 128, 128)) < 0.5))
    res["dense_noise"] = case(volume)
    res["scratch_bytes"] = volume.editScratchBytes()
    volume.close()
    return res


def bench_depth(vrc, depth, pairs):
    import torch
    S = 1 << depth
    rng = np.random.default_rng(depth)
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    res = {"size": S, "nodes": scene.n_nodes}
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        volume = vrc.VoxelVolume.fromScene(scene)
        walls.append((time.perf_counter() - t0) * 1e3)
        if _ < 2:
            volume.close()
    res["from_scene_ms"] = round(statistics.median(walls), 4)
    scene.close()
    res["solid_voxels"] = volume.solidCount()

    # commit against the one-shot builder on the same occupancy (the untouched terrain), A B A B
    dense = volume.download()
    commit, build = [], []
    for i in range(pairs + 1):
        a = volume.commit()
        b = vrc.LSVO.fromVolume(dense, depth)
        assert a.n_nodes == b.n_nodes
        if i:
            commit.append(a.build_ms)
            build.append(b.build_ms)
        a.close()
        b.close()
    res["commit_ms"], res["build_volume_ms"] = stat(commit, 4), stat(build, 4)
    res["commit_within_baseline_spread"] = bool(statistics.median(commit) <= max(build))
    res["pairs"] = pairs

    # edits: device memory, the NULL stream (where torch's events are recorded)
    res["set_voxels_ms"] = {}
    for n in (1, 1000, 1000000):
        xyz = torch.from_numpy(rng.integers(0, S, (n, 3)).astype(np.int32)).cuda()
        flip = [False]

        def one():
            flip[0] = not flip[0]
            volume.setVoxelsDevice(n, xyz.data_ptr(), flip[0], None)
        device_ms(one, 2)
        res["set_voxels_ms"][str(n)] = round(device_ms(one, 5), 5)
    lo = S // 2 - 32
    box = torch.tensor([lo, lo, lo, lo + 64, lo + 64, lo + 64], dtype=torch.int32).cuda()
    res["fill_box_64_ms"] = round(device_ms(lambda: volume.fillBoxesDevice(1, box.data_ptr(), True, None)), 5)
    volume.close()
    return res


def bench_components(vrc, depth, pairs):
    import torch
    S = 1 << depth
    rng = np.random.default_rng(depth)
    res = {"size": S, "pairs": pairs, "id_array_bytes": 4 * S ** 3}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)

    def case(medium, connectivity, through_empty):
        r = {"connectivity": connectivity, "through_empty": through_empty}
        r["label_ms"], labels = timed(lambda: medium.labelComponents(connectivity, through_empty), pairs)
        walls = []
        for i in range(pairs + 1):
            t0 = time.perf_counter()
            rec = labels.components()
            if i:
                walls.append((time.perf_counter() - t0) * 1e3)
        r["records_wall_ms"] = stat(walls, 4)
        r["pieces"], r["largest"], r["voxels"] = len(rec), int(rec["voxels"].max()), int(rec["voxels"].sum(dtype=np.uint64))
        r["labels_bytes"] = labels.bytes()
        dst = vrc.VoxelVolume(depth)
        one = np.zeros(len(rec), np.uint8)
        one[int(np.argmax(rec["voxels"]))] = 1
        t_one, t_all = torch.from_numpy(one).cuda(), torch.ones(len(rec), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        r["select_one_ms"], _ = timed(lambda: labels.selectDevice(t_one.data_ptr(), dst), pairs)
        assert dst.solidCount() == r["largest"]
        r["select_all_ms"], _ = timed(lambda: labels.selectDevice(t_all.data_ptr(), dst), pairs)
        assert dst.solidCount() == r["voxels"]
        dst.close()
        if not through_empty:
            walls = []
            for i in range(pairs + 1):
                clone = medium.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, removed = clone.removeSmallPieces(8, connectivity)
                torch.cuda.synchronize()
                if i:
                    walls.append((time.perf_counter() - t0) * 1e3)
                clone.close()
            r["remove_small_8_wall_ms"], r["remove_small_8_pieces"] = stat(walls, 3), removed
        labels.close()
        return r, rec

    res["terrain"], _ = case(terrain, 6, False)
    cam = np.array(vrc.reference_camera_position(depth), np.float32) / np.float32(S) + np.float32(1.0)
    d = rng.normal(size=(400, 3)).astype(np.float32) * np.float32(0.3) + np.array([0.0, 0.5, 0.8], np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    hits = scene.castRays(np.tile(cam, (400, 1)).astype(np.float32), d)
    terrain.fillSpheresAtHits(hits, 12, False)
    res["digs"] = {"rays": 400, "unit_hits": int(((hits["hit"] & 0xff) == 1).sum()), "radius": 12}
    res["dug_terrain"], rec = case(terrain, 6, False)
    res["dug_terrain_26"], _ = case(terrain, 26, False)
    res["air"], _ = case(terrain, 6, True)

    # for scale, same run, same volume
    scale = {}
    ids = torch.empty(S ** 3, dtype=torch.int32, device="cuda")
    scale["fill_ids_ms"], _ = timed(lambda: ids.fill_(7), pairs)
    del ids
    scale["solid_count_ms"], _ = timed(terrain.solidCount, pairs)
    region = vrc.VoxelVolume(depth)
    whole = np.array([[0, 0, 0, S, S, S]], np.uint32)

    def flood_from(seed_boxes=None, seed_voxel=None):
        region.fillBoxes(whole, False)
        if seed_boxes is not None:
            region.fillBoxes(seed_boxes)
        else:
            region.setVoxels([seed_voxel])
        ms, st = event_ms(lambda: region.flood(terrain, 6))
        assert st.converged == 1
        return ms, st

    bottom = np.array([[0, S // 2 + 1, 0, S, S // 2 + 2, S]], np.uint32)
    floods = [flood_from(seed_boxes=bottom)[0] for _ in range(pairs + 1)][1:]
    scale["flood_from_bottom_ms"] = stat(floods, 4)
    flood_from(seed_voxel=rec[0]["first"])                                   # warm-up
    largest = np.argsort(-rec["voxels"].astype(np.int64), kind="stable")[:16]
    per_piece = []
    for i in largest:
        ms, st = flood_from(seed_voxel=rec[int(i)]["first"])
        assert st.reached == int(rec[int(i)]["voxels"])
        per_piece.append(ms)
    scale["flood_per_piece"] = {"pieces_flooded": len(per_piece), "each_ms": stat(per_piece, 4), "sum_ms": round(sum(per_piece), 4),
                                "pieces": len(rec),
                                "all_pieces_ms_EXTRAPOLATED": round(statistics.mean(per_piece) * len(rec), 3),
                                "note": "extrapolated: mean of the floods made x number of pieces; host round trips to find the seeds not included"}
    label = res["dug_terrain"]["label_ms"]["median"]
    scale["label_over_fill_ids"] = round(label / scale["fill_ids_ms"]["median"], 2)
    scale["flood_per_piece_EXTRAPOLATED_over_label"] = round(scale["flood_per_piece"]["all_pieces_ms_EXTRAPOLATED"] / label, 2)
    res["scale"] = scale
    region.close()
    terrain.close()
    scene.close()
    return res


def bench_distance(vrc, depth, pairs):
    import torch
    S = 1 << depth
    res = {"size": S, "pairs": pairs, "field_bytes": 4 * S ** 3}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    corner = vrc.VoxelVolume(depth)
    corner.setVoxels([[0, 0, 0]])
    empty = vrc.VoxelVolume(depth)

    src = torch.empty(S ** 3, dtype=torch.int32, device="cuda")
    dst_t = torch.empty(S ** 3, dtype=torch.int32, device="cuda")
    res["copy_field_ms"], _ = timed(lambda: dst_t.copy_(src), pairs)
    del src, dst_t
    torch.cuda.empty_cache()
    copy = res["copy_field_ms"]["median"]

    for name, medium in (("terrain", terrain), ("corner_voxel", corner), ("empty", empty)):
        res[name] = {}
        for to_empty in (False, True):
            r = {}
            r["field_ms"], field = timed(lambda: medium.distanceField(to_empty), pairs)
            r["features"], r["max_d2"], r["argmax"] = int(field.stats.features), int(field.stats.max_d2), [int(v) for v in field.stats.argmax]
            dst = vrc.VoxelVolume(depth)
            r["select_ms"], _ = timed(lambda: field.select(0, 16, dst) and None, pairs)      # select returns dst: not timed()'s to close
            r["selected"] = dst.solidCount()
            dst.close()
            field.close()
            walls = []
            for i in range(pairs + 1):
                clone = medium.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                clone.dilate(4)
                torch.cuda.synchronize()
                if i:
                    walls.append((time.perf_counter() - t0) * 1e3)
                grown = clone.solidCount()
                clone.close()
            r["dilate_4_wall_ms"], r["dilate_4_solid"] = stat(walls, 3), grown
            r["field_over_copy"] = round(r["field_ms"]["median"] / copy, 2)
            res[name]["to_empty" if to_empty else "to_solid"] = r
    res["worst_over_terrain"] = {k: round(res["corner_voxel"][k]["field_ms"]["median"] / res["terrain"][k]["field_ms"]["median"], 2)
                                 for k in ("to_solid", "to_empty")}
    for v in (terrain, corner, empty):
        v.close()
    scene.close()
    return res


def bench_travel(vrc, depth, pairs):
    """vrc_travel_field on the FastNoise terrain: through the air from one seed voxel above the ground and through
    the solid from the floor layer (the slab y = S / 2 + 1 its columns stand on), both connectivities; device ms by events, median of `pairs`, and the sweeps
    issued.  In the same run vrc_volume_flood from the same seeds on the same medium: it computes the support of the same
    field (a fresh copy of the seeds per repeat, made outside the timed span)."""
    S = 1 << depth
    res = {"size": S, "pairs": pairs, "field_bytes": 4 * S ** 3}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    # the slab the terrain's columns stand on (the flood mode's `bottom`), and the highest empty voxel of the centre column
    floor_y = S // 2 + 1
    above = next(([S // 2, y, S // 2] for y in range(S - 2, -1, -1) if not terrain.getVoxels([[S // 2, y, S // 2]])[0]), None)
    if above is None:
        raise SystemExit("bench_travel: no empty voxel in the column at the centre of the terrain")
    air_seed = vrc.VoxelVolume(depth)
    air_seed.setVoxels([above])
    floor = vrc.VoxelVolume(depth)
    floor.fillBoxes([[0, floor_y, 0, S, floor_y + 1, S]])

    def count_reached(stats, region):
        reached = region.solidCount()
        region.close()
        return stats, reached

    for name, seeds, through_empty in (("air_from_one_seed", air_seed, True), ("solid_from_the_floor", floor, False)):
        res[name] = {"seed": above if seeds is air_seed else "layer y = %d" % floor_y}
        for connectivity in (6, 26):
            r = {}
            r["travel_ms"], field = timed(lambda: terrain.travelField(seeds, connectivity, through_empty), pairs)
            st = field.stats
            r["seeds"], r["reached"], r["max_steps"], r["sweeps"] = int(st.seeds), int(st.reached), int(st.max_steps), int(st.sweeps)
            field.close()
            r["flood_ms"], (fst, flooded) = timed(lambda region: region.flood(terrain, connectivity, through_empty), pairs, before=seeds.clone, after=count_reached)
            r["flood_sweeps"], r["flood_reached"] = int(fst.sweeps), int(flooded)
            r["travel_over_flood"] = round(r["travel_ms"]["median"] / r["flood_ms"]["median"], 2)
            res[name]["connectivity_%d" % connectivity] = r
    for v in (terrain, air_seed, floor):
        v.close()
    scene.close()
    return res


def bench_fall(vrc, depth, pairs):
    """vrc_fall_drops / vrc_fall_place on the FastNoise terrain with a band carved out (see the module's text), next to
    vrc_volume_label_components and vrc_labels_select of the same debris in the same run."""
    import torch
    S = 1 << depth
    res = {"size": S, "pairs": pairs}
    scene, world, debris, _, _ = fall_scene(vrc, depth, label=False)           # the labelling is timed below
    res["band"], res["supported_voxels"], res["debris_voxels"] = fall_cuts(S)[0][0], world.solidCount(), debris.solidCount()
    down = vrc.capi.VRC_FACE_YN
    res["label_ms"], labels = timed(lambda: debris.labelComponents(6), pairs)
    res["pieces"] = labels.count
    offsets = torch.zeros((max(labels.count, 1), 3), dtype=torch.int32).cuda()
    keep = torch.ones(max(labels.count, 1), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    res["fall_ms"], st = timed(lambda: labels.fallDevice(offsets.data_ptr(), world, down), pairs)
    res["rounds"], res["moved_pieces"], res["moved_voxels"], res["max_drop"] = int(st.rounds), int(st.moved_pieces), int(st.moved_voxels), int(st.max_drop)
    res["fall_round_over_label"] = round(res["fall_ms"]["median"] / max(st.rounds, 1) / res["label_ms"]["median"], 3)
    target = world.clone()
    res["place_ms"], _ = timed(lambda: labels.placeDevice(offsets.data_ptr(), target, vrc.capi.VRC_COPY_OR, None, None) and None, pairs)
    res["placed_voxels"] = target.solidCount()
    res["select_ms"], _ = timed(lambda: labels.selectDevice(keep.data_ptr(), target, vrc.capi.VRC_COPY_OR, None), pairs)
    for v in (labels, target, debris, world):
        v.close()
    scene.close()
    return res


def bench_rigid(vrc, depth, pairs):
    """vrc_rigid_moments next to vrc_labels_select, vrc_rigid_place_affine next to vrc_fall_place, on fall_scene"""
    import torch
    S = 1 << depth
    res = {"size": S, "pairs": pairs}
    scene, world, debris, labels, _ = fall_scene(vrc, depth)
    C_ = labels.count
    res["pieces"], res["supported_voxels"], res["debris_voxels"] = C_, world.solidCount(), debris.solidCount()
    OR = vrc.capi.VRC_COPY_OR

    keep = torch.ones(max(C_, 1), dtype=torch.uint8).cuda()
    moments = torch.zeros(max(C_, 1) * 80, dtype=torch.uint8).cuda()
    target = world.clone()
    torch.cuda.synchronize()
    res["moments_ms"], _ = timed(lambda: labels.momentsDevice(0, C_, moments.data_ptr(), None), pairs)
    res["select_ms"], _ = timed(lambda: labels.selectDevice(keep.data_ptr(), target, OR, None), pairs)
    res["moments_over_select"] = round(res["moments_ms"]["median"] / res["select_ms"]["median"], 2)
    got = moments.cpu().numpy().view(vrc.capi.MOMENTS_DTYPE)[:C_]
    records = labels.components()
    assert np.array_equal(got["voxels"], records["voxels"]) and int(got["voxels"].sum()) == res["debris_voxels"]
    res["largest_piece_voxels"] = int(got["voxels"].max(initial=0))

    offsets, st = labels.fall(world, vrc.capi.VRC_FACE_YN)
    res["max_drop"] = int(st.max_drop)
    maps, boxes = translate_poses(labels, records, offsets, S)
    res["translate_box_words"] = box_words(boxes)
    d_offsets, d_maps, d_boxes = on_device(offsets), on_device(maps), on_device(boxes)
    by_fall, by_maps = world.clone(), world.clone()
    torch.cuda.synchronize()
    # the place calls return their destination: `and None` keeps timed() from closing it
    res["fall_place_ms"], _ = timed(lambda: labels.placeDevice(d_offsets.data_ptr(), by_fall, OR, None, None) and None, pairs)
    res["place_translate_ms"], _ = timed(lambda: labels.placeAffineDevice(d_maps.data_ptr(), by_maps, d_boxes.data_ptr(), OR, None, None) and None, pairs)
    res["place_translate_over_fall_place"] = round(res["place_translate_ms"]["median"] / res["fall_place_ms"]["median"], 2)
    res["placed_voxels"] = by_maps.solidCount()
    assert res["placed_voxels"] == by_fall.solidCount() and np.array_equal(by_maps.download(), by_fall.download()), "translation maps differ from vrc_fall_place"

    maps, boxes = turn_poses(labels)
    d_maps, d_boxes = on_device(maps), on_device(boxes)
    turned = world.clone()
    torch.cuda.synchronize()
    res["place_turn_ms"], _ = timed(lambda: labels.placeAffineDevice(d_maps.data_ptr(), turned, d_boxes.data_ptr(), OR, None, None) and None, pairs)
    res["turned_voxels"] = turned.solidCount()
    res["turn_box_words"] = box_words(boxes)
    for v in (turned, by_fall, by_maps, target, labels, debris, world):
        v.close()
    scene.close()
    return res


def bench_contacts(vrc, depth, pairs):
    """vrc_rigid_contacts next to vrc_rigid_place_affine with the same maps and boxes, on fall_scene"""
    import torch
    S = 1 << depth
    res = {"size": S, "pairs": pairs}
    scene, world, debris, labels, full = fall_scene(vrc, depth, whole=True)       # full: the supported part and the debris
    C_ = labels.count
    res["pieces"], res["supported_voxels"], res["debris_voxels"] = C_, world.solidCount(), debris.solidCount()
    OR = vrc.capi.VRC_COPY_OR

    records = labels.components()
    offsets, st = labels.fall(world, vrc.capi.VRC_FACE_YN)
    maps, boxes = translate_poses(labels, records, offsets, S)
    turn_maps, turn_boxes = turn_poses(labels)
    out = torch.zeros(max(C_, 1) * 128, dtype=torch.uint8).cuda()
    for name, mp, bx in (("translate", maps, boxes), ("turn", turn_maps, turn_boxes)):
        d_maps, d_boxes = on_device(mp), on_device(bx)
        placed = world.clone()
        torch.cuda.synchronize()
        res[name + "_box_words"] = box_words(bx)
        # the place call returns its destination: `and None` keeps timed() from closing it
        res["place_%s_ms" % name], _ = timed(lambda: labels.placeAffineDevice(d_maps.data_ptr(), placed, d_boxes.data_ptr(), OR, None, None) and None, pairs)
        for suffix, against in (("", world), ("_full", full)):
            key = "contacts_%s%s" % (name, suffix)
            res[key + "_ms"], _ = timed(lambda: labels.contactsDevice(d_maps.data_ptr(), against, out.data_ptr(), d_boxes.data_ptr(), None, None), pairs)
            res[key + "_over_place"] = round(res[key + "_ms"]["median"] / res["place_%s_ms" % name]["median"], 2)
            got = out.cpu().numpy().view(vrc.capi.CONTACT_DTYPE)[:C_]
            assert got.tobytes() == labels.contacts(mp, against, bx).tobytes(), "device-memory records differ from the host-memory call's"
            res[key] = {"posed_voxels": int(got["posed"].sum()), "overlap_voxels": int(got["overlap"].sum()), "touch_voxels": int(got["touch"].sum()),
                        "pieces_overlapping": int((got["overlap"] > 0).sum()), "pieces_touching": int((got["touch"] > 0).sum())}
        placed.close()
    assert res["contacts_translate"]["overlap_voxels"] == 0 and res["contacts_translate"]["posed_voxels"] == res["debris_voxels"], "the fall's offsets overlap the supported part"
    for v in (labels, debris, full, world):
        v.close()
    scene.close()
    return res


def bench_clearance(vrc, depth, pairs):
    """vrc_rigid_clearance over the Euclidean field of the supported part next to vrc_rigid_contacts against the supported part
    with the same maps and boxes -- the same gather, reading at most 7 words where the clearance reads up to 32 values -- on
    fall_scene, A B A B in one run"""
    import torch
    S = 1 << depth
    res = {"size": S, "pairs": pairs}
    scene, world, debris, labels, _ = fall_scene(vrc, depth)
    field = world.distanceField(False, False)
    C_ = labels.count
    res["pieces"], res["supported_voxels"], res["debris_voxels"] = C_, world.solidCount(), debris.solidCount()

    records = labels.components()
    offsets, st = labels.fall(world, vrc.capi.VRC_FACE_YN)
    maps, boxes = translate_poses(labels, records, offsets, S)
    turn_maps, turn_boxes = turn_poses(labels)
    out = torch.zeros(max(C_, 1) * 64, dtype=torch.uint8).cuda()
    contact_out = torch.zeros(max(C_, 1) * 128, dtype=torch.uint8).cuda()
    for name, mp, bx in (("translate", maps, boxes), ("turn", turn_maps, turn_boxes)):
        d_maps, d_boxes = on_device(mp), on_device(bx)
        torch.cuda.synchronize()
        res[name + "_box_words"] = box_words(bx)
        res["clearance_%s_ms" % name], res["contacts_%s_ms" % name] = ab_device_ms(
            lambda: labels.clearanceDevice(d_maps.data_ptr(), field, out.data_ptr(), d_boxes.data_ptr(), None, None),
            lambda: labels.contactsDevice(d_maps.data_ptr(), world, contact_out.data_ptr(), d_boxes.data_ptr(), None, None), pairs)
        res["clearance_%s_over_contacts" % name] = round(res["clearance_%s_ms" % name]["median"] / res["contacts_%s_ms" % name]["median"], 2)
        got = out.cpu().numpy().view(vrc.capi.CLEARANCE_DTYPE)[:C_]
        assert got.tobytes() == labels.clearance(mp, field, bx).tobytes(), "device-memory records differ from the host-memory call's"
        hit = contact_out.cpu().numpy().view(vrc.capi.CONTACT_DTYPE)[:C_]
        assert np.array_equal(got["posed"], hit["posed"]) and np.array_equal(got["min_value"] == 0, hit["overlap"] > 0), "clearance and contacts disagree"
        finite = got["min_value"] != vrc.capi.VRC_DISTANCE_NONE
        res["clearance_" + name] = {"posed_voxels": int(got["posed"].sum()), "pieces_posed": int((got["posed"] > 0).sum()),
                                    "pieces_overlapping": int((got["min_value"] == 0).sum()), "pieces_within_one_voxel": int((got["min_value"] == 1).sum()),
                                    "largest_min_value": int(got["min_value"][finite].max(initial=0)), "largest_max_value": int(got["max_value"].max(initial=0))}
    assert res["clearance_translate"]["pieces_overlapping"] == 0 and res["clearance_translate"]["posed_voxels"] == res["debris_voxels"], "the fall's offsets overlap the supported part"
    for v in (field, labels, debris, world):
        v.close()
    scene.close()
    return res


def bench_pair_contacts(vrc, depth, pairs):
    """vrc_rigid_box_pairs + vrc_rigid_pair_contacts on fall_scene with turn_poses (bench_contacts' turned poses), next to the
    documented workaround on a sample of the pairs: vrc_rigid_place_affine of b alone into a cleared scratch volume, then
    vrc_rigid_contacts of a alone against it"""
    import ctypes as C
    import torch
    S = 1 << depth
    res = {"size": S, "pairs": pairs}
    scene, world, debris, labels, _ = fall_scene(vrc, depth)
    C_ = labels.count
    res["pieces"], res["debris_voxels"] = C_, debris.solidCount()
    L, DEV, OR = vrc.capi.load(), vrc.capi.VRC_MEM_DEVICE, vrc.capi.VRC_COPY_OR

    maps, boxes = turn_poses(labels)
    d_maps, d_boxes = on_device(maps), on_device(boxes)
    listed = labels.candidatePairs(boxes)
    P = len(listed)
    res["candidate_pairs"] = P
    d_pairs = torch.zeros(max(P, 1) * 8, dtype=torch.uint8).cuda()
    out = torch.zeros(max(P, 1) * 128, dtype=torch.uint8).cuda()
    count = C.c_uint64()
    torch.cuda.synchronize()

    def broad():
        vrc.capi.check(L.vrc_rigid_box_pair_count(labels._h, None, vrc.capi.ptr(d_boxes.data_ptr()), depth, C.byref(count), DEV, None))
        vrc.capi.check(L.vrc_rigid_box_pairs(labels._h, None, vrc.capi.ptr(d_boxes.data_ptr()), depth, 0, P, vrc.capi.ptr(d_pairs.data_ptr()), DEV, None))

    # both calls are synchronous and allocate their scratch: the events span that too
    res["box_pairs_count_and_list_ms"], _ = timed(broad, pairs)
    assert count.value == P and d_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2)[:P].tobytes() == listed.tobytes()
    res["pair_contacts_ms"], _ = timed(lambda: labels.pairContactsDevice(d_maps.data_ptr(), P, d_pairs.data_ptr(), out.data_ptr(), d_boxes.data_ptr(), depth, None, None), pairs)
    got = out.cpu().numpy().view(vrc.capi.CONTACT_DTYPE)[:P]
    assert got.tobytes() == labels.pairContacts(maps, listed, boxes).tobytes(), "device-memory records differ from the host-memory call's"
    res["pairs_overlapping"], res["pairs_touching"] = int((got["overlap"] > 0).sum()), int((got["touch"] > 0).sum())
    res["overlap_voxels"], res["touch_voxels"] = int(got["overlap"].sum()), int(got["touch"].sum())
    # the yardstick: per pair one placement of b alone into a cleared scratch volume and one contact call of a alone against it
    sample = listed[:: max(1, P // 64)][:64]
    res["yardstick_sample_pairs"] = len(sample)
    scratch = vrc.VoxelVolume(depth)
    whole = [[0, 0, 0, S, S, S]]
    keeps = torch.zeros((2, max(C_, 1)), dtype=torch.uint8).cuda()
    one = torch.zeros(max(C_, 1) * 128, dtype=torch.uint8).cuda()
    times = []
    for a, b in sample.tolist():
        keeps.zero_()
        keeps[0, b], keeps[1, a] = 1, 1
        torch.cuda.synchronize()

        def workaround():
            scratch.fillBoxes(whole, False)
            labels.placeAffineDevice(d_maps.data_ptr(), scratch, d_boxes.data_ptr(), OR, keeps[0].data_ptr(), None)
            labels.contactsDevice(d_maps.data_ptr(), scratch, one.data_ptr(), d_boxes.data_ptr(), keeps[1].data_ptr(), None)
        times.append(timed(workaround, pairs)[0]["median"])
        # away from the volume's faces the workaround's record is the pair's; at the faces it also counts the walls
        rec = one.cpu().numpy().view(vrc.capi.CONTACT_DTYPE)[a]
        k = int(np.flatnonzero((listed[:, 0] == a) & (listed[:, 1] == b))[0])
        assert rec["posed"] == got[k]["posed"] and rec["overlap"] == got[k]["overlap"], "the workaround disagrees with the pair call"
    res["yardstick_per_pair_ms"] = stat(times, 4)
    res["yardstick_scaled_ms"] = round(res["yardstick_per_pair_ms"]["median"] * P, 2)
    res["yardstick_over_pair_contacts"] = round(res["yardstick_scaled_ms"] / res["pair_contacts_ms"]["median"], 1)
    res["not_timed_apart"] = "the zeroing of the records, the two gathers and the reduction of vrc_rigid_pair_contacts; the count, scan and emit passes and the " \
                             "scratch allocation of the broad phase; the clearing, the placement and the contact call of the workaround"
    for v in (scratch, labels, debris, world):
        v.close()
    scene.close()
    return res


def bench_stamp(vrc, depth, pairs):
    S = 1 << depth
    res = {"size": S, "pairs": pairs}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    copied, stamped = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
    REPLACE = vrc.capi.VRC_COPY_REPLACE
    whole = ([0, 0, 0], [S, S, S], [0, 0, 0])
    identity = vrc.make_affine([65536, 0, 0, 0, 65536, 0, 0, 0, 65536], [0, 0, 0])

    def copy():
        copied.copyRegion(terrain, *whole, REPLACE, None)

    a, b = ab_device_ms(copy, lambda: stamped.stampAffine(terrain, identity, None, None, REPLACE, None), pairs)
    same = bool(np.array_equal(copied.download(), stamped.download())) if depth <= 9 else copied.solidCount() == stamped.solidCount()
    assert same and copied.solidCount() == stamped.solidCount() == terrain.solidCount(), "identity stamp differs from vrc_volume_copy_region"
    res["identity"] = {"copy_region_ms": a, "stamp_ms": b, "stamp_over_copy": round(b["median"] / a["median"], 2), "equal": same,
                       "solid": stamped.solidCount()}

    turn = vrc.affine_signed_permutation((1, 0, 2), (0, 1, 0), S)
    a, b = ab_device_ms(copy, lambda: stamped.stampAffine(terrain, turn, None, None, REPLACE, None), pairs)
    res["quarter_turn"] = {"copy_region_ms": a, "stamp_ms": b, "stamp_over_copy": round(b["median"] / a["median"], 2), "solid": stamped.solidCount()}

    rot = turn_30_30()
    placed, lo, hi = vrc.affine_place(rot, 1.0, (S / 2,) * 3, (S / 2,) * 3, depth, depth)
    a, b = ab_device_ms(copy, lambda: stamped.stampAffine(terrain, placed, lo, hi, REPLACE, None), pairs)
    res["turn_30_30"] = {"copy_region_ms": a, "stamp_ms": b, "stamp_over_copy": round(b["median"] / a["median"], 2), "box": [list(lo), list(hi)],
                         "solid": stamped.solidCount()}

    clip = vrc.VoxelVolume(6)
    clip.copyRegion(terrain, [S // 2 - 32, S // 2 - 16, S // 2 - 32], [64, 64, 64], [0, 0, 0], REPLACE, None)
    placed, lo, hi = vrc.affine_place(rot, 2.0, (32.0,) * 3, (S / 2,) * 3, 6, depth)
    m = S // 2 - 64
    a, b = ab_device_ms(lambda: copied.copyRegion(terrain, [m, m, m], [128, 128, 128], [m, m, m], REPLACE, None),
                        lambda: stamped.stampAffine(clip, placed, lo, hi, vrc.capi.VRC_COPY_OR, None), pairs)
    res["clipboard_64_x2"] = {"copy_128_ms": a, "stamp_ms": b, "stamp_over_copy": round(b["median"] / a["median"], 2), "box": [list(lo), list(hi)],
                              "clipboard_solid": clip.solidCount(), "solid": stamped.solidCount()}
    for v in (clip, stamped, copied, terrain):
        v.close()
    scene.close()
    return res


def bench_fracture(vrc, depth, pairs):
    """vrc_fracture_label on the FastNoise terrain next to vrc_volume_distance_field plus vrc_volume_label_components of the
    same medium (the yardstick: the same traffic plus the index), A B A B in one run; see the module's text."""
    import torch
    from cpuvoxelraycaster_amd import scenes
    S = 1 << depth
    res = {"size": S, "pairs": pairs}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    world = vrc.VoxelVolume.fromScene(scene)
    res["solid_voxels"] = world.solidCount()
    x = z = S // 2
    column = world.getVoxels(np.stack([np.full(S, x), np.arange(S), np.full(S, z)], axis=1).astype(np.uint32))
    top = int(np.flatnonzero(column).max())
    rng = np.random.default_rng(4096)
    cases = {"impact_64_sites_radius_48": (scenes.scatter_sites((x, top, z), 48, 64, 64), 48),
             "whole_volume_4096_sites": (rng.integers(0, S, (4096, 3)).astype(np.int32), None)}

    def yardstick():
        field = world.distanceField()
        labels = world.labelComponents(6)
        field.close()
        return labels

    for name, (sites, radius) in cases.items():
        t_sites = torch.from_numpy(np.ascontiguousarray(sites)).cuda()
        torch.cuda.synchronize()
        a_ms, b_ms, pieces = [], [], 0
        for i in range(pairs + 1):                                         # one warm-up pair, then A B A B
            ms, labels = event_ms(lambda: world.fractureDevice(len(sites), t_sites.data_ptr(), 6, False, radius))
            pieces, shards = labels.count, int((labels.pieceSites() != vrc.capi.VRC_NO_COMPONENT).sum())
            labels.close()
            if i:
                a_ms.append(ms)
            ms, labels = event_ms(yardstick)
            plain = labels.count
            labels.close()
            if i:
                b_ms.append(ms)
        res[name] = {"sites": len(sites), "max_distance": radius, "pieces": pieces, "shards": shards, "plain_pieces": plain,
                     "fracture_ms": stat(a_ms, 4), "distance_plus_label_ms": stat(b_ms, 4),
                     "fracture_over_distance_plus_label": round(stat(a_ms, 4)["median"] / stat(b_ms, 4)["median"], 3)}
    world.close()
    scene.close()
    return res


def bench_delta(vrc, depth, pairs):
    """vrc_delta_diff next to vrc_volume_clone and vrc_delta_apply next to a copy of one occupancy; see the module's text."""
    import torch
    S = 1 << depth
    occupancy = S ** 3 // 8
    res = {"size": S, "pairs": pairs, "occupancy_bytes": occupancy}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    x = z = S // 2
    column = terrain.getVoxels(np.stack([np.full(S, x), np.arange(S), np.full(S, z)], axis=1).astype(np.uint32))
    surface_y = int(np.flatnonzero(column).max())            # the terrain's relief, as --fracture finds it
    t_src, t_dst = torch.zeros(occupancy, dtype=torch.uint8).cuda(), torch.zeros(occupancy, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()

    def case(before, after):
        delta = before.diff(after)
        st = delta.stats
        one = {"records": delta.count, "record_bytes": delta.bytes(), "record_bytes_over_occupancy": round(delta.bytes() / occupancy, 6),
               "changed_voxels": int(st.voxels), "box": [list(st.lo), list(st.hi)]}
        one["diff_ms"], one["clone_ms"] = timed_ab([lambda: before.diff(after), before.clone], pairs, digits=4)
        one["diff_over_clone"] = round(one["diff_ms"]["median"] / one["clone_ms"]["median"], 3)

        def apply_twice():
            before.applyDelta(delta)
            before.applyDelta(delta)

        def copy():
            t_dst.copy_(t_src)

        twice, one["copy_ms"] = timed_ab([apply_twice, copy], pairs, digits=4)
        one["apply_ms"] = {k: round(v / 2, 5) for k, v in twice.items()}
        one["diff_over_copy"] = round(one["diff_ms"]["median"] / one["copy_ms"]["median"], 3)
        check = before.diff(after)
        assert check.count == delta.count and check.records().tobytes() == delta.records().tobytes(), "the applies did not leave `before` as it was"
        check.close()
        delta.close()
        return one

    dug = terrain.clone()
    dug.fillSpheres([(x, surface_y, z, 8)], False)
    res["sphere_dig_r8"] = case(terrain, dug)
    dug.close()

    world = terrain.clone()                                  # fall_scene's medium, from the terrain already here
    cuts, slab = fall_cuts(S)
    world.fillBoxes(cuts, False)
    carved = world.clone()
    fall = world.dropLoose(slab, vrc.capi.VRC_FACE_YN)
    res["drop_loose"] = dict(case(carved, world), moved_pieces=int(fall.moved_pieces), moved_voxels=int(fall.moved_voxels))
    for v in (carved, world):
        v.close()

    empty = vrc.VoxelVolume(depth)
    res["terrain_vs_empty"] = case(terrain, empty)
    for v in (empty, terrain):
        v.close()
    scene.close()
    return res


def bench_pack(vrc, depth, pairs):
    """vrc_pack_volume / vrc_unpack_volume next to vrc_volume_clone and vrc_volume_download; see the module's text."""
    import ctypes as C
    import torch
    capi = vrc.capi
    L = capi.load()
    S = 1 << depth
    res = {"size": S, "rounds": pairs, "occupancy_bytes": S ** 3 // 8, "dense_bytes": S ** 3, "bound_bytes": int(L.vrc_pack_bound(depth))}
    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    noise = vrc.VoxelVolume(depth)
    noise.fillRandom(1, 0.5)
    dense = np.zeros((S, S, S), np.uint8)
    for name, volume in (("terrain", terrain), ("random_half", noise)):
        info = volume.packInfo()
        n = int(info.bytes)
        one = {"stream_bytes": n, "mixed_tiles": int(info.mixed_tiles), "full_tiles": int(info.full_tiles), "tiles": int(info.tiles),
               "partial_bricks": int(info.partial_bricks), "solid": int(info.solid), "stream_over_occupancy": round(n / (S ** 3 // 8), 4),
               "stream_over_dense": round(n / S ** 3, 5)}
        buf = torch.empty(n, dtype=torch.uint8, device="cuda")
        target = vrc.VoxelVolume(depth)
        scratch = capi.PackInfo()

        def size_only():
            capi.check(L.vrc_pack_volume(volume._h, None, 0, C.byref(scratch), capi.VRC_MEM_DEVICE))

        def pack():
            capi.check(L.vrc_pack_volume(volume._h, capi.ptr(buf.data_ptr()), n, C.byref(scratch), capi.VRC_MEM_DEVICE))

        def unpack():
            capi.check(L.vrc_unpack_volume(target._h, capi.ptr(buf.data_ptr()), n, capi.VRC_MEM_DEVICE))

        def download():
            capi.check(L.vrc_volume_download(volume._h, capi.ptr(dense)))

        calls = [("size_ms", size_only), ("pack_ms", pack), ("unpack_ms", unpack), ("clone_ms", volume.clone), ("download_ms", download)]
        one.update(zip([key for key, _ in calls], timed_ab([fn for _, fn in calls], pairs, digits=4)))
        assert target.pack().tobytes() == volume.pack().tobytes(), "the unpacked volume does not pack to the same stream"
        target.close()
        res[name] = one
    for v in (noise, terrain):
        v.close()
    scene.close()
    return res


def bench_cells(vrc, depth, pairs):
    """vrc_cells_step and vrc_cells_fill_random next to vrc_volume_copy_region and vrc_volume_clone; see the module's text."""
    import torch
    S = 1 << depth
    CALLS = 20                           # a single call is tens of microseconds: a sample times twenty in a row
    res = {"size": S, "pairs": pairs, "calls_per_sample": CALLS, "occupancy_bytes": S ** 3 // 8}
    counter = torch.zeros(1, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    birth26, survive26 = vrc.count_mask(range(14, 27)), vrc.count_mask(range(13, 27))
    rules = {6: (0, vrc.count_mask(range(1, 7))), 26: (birth26, survive26)}

    def case(src):
        dst, other = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
        one = {"solid_voxels": src.solidCount()}

        def copy():
            other.copyRegion(src, (0, 0, 0), (S, S, S), (0, 0, 0))

        for neighbours, (birth, survive) in rules.items():
            key = "step_%d" % neighbours
            one[key] = {}
            one[key]["ms"], one[key]["copy_region_ms"] = timed_ab([lambda: src.cellStepDevice(dst, birth, survive, None, neighbours), copy], pairs, CALLS)
            one[key]["step_over_copy"] = round(one[key]["ms"]["median"] / one[key]["copy_region_ms"]["median"], 3)
            key += "_changed"
            one[key] = {}
            one[key]["ms"], one[key]["clone_ms"] = timed_ab([lambda: src.cellStepDevice(dst, birth, survive, counter.data_ptr(), neighbours), src.clone], pairs, CALLS)
            one[key]["changed"] = int(counter.cpu()[0])
            one[key]["step_over_clone"] = round(one[key]["ms"]["median"] / one[key]["clone_ms"]["median"], 3)
        one["fill_random"] = {}
        one["fill_random"]["ms"], one["fill_random"]["copy_region_ms"] = timed_ab([lambda: dst.fillRandom(7, 0.5, None, vrc.capi.VRC_COPY_REPLACE) and None, copy], pairs, CALLS)
        one["fill_random"]["fill_over_copy"] = round(one["fill_random"]["ms"]["median"] / one["fill_random"]["copy_region_ms"]["median"], 3)
        for v in (dst, other):
            v.close()
        return one

    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    res["terrain"] = case(terrain)
    terrain.close()
    scene.close()
    noise = vrc.VoxelVolume(depth).fillRandom(1337, 0.5, None, vrc.capi.VRC_COPY_REPLACE)
    res["random_0.5"] = case(noise)
    noise.close()
    return res


def bench_columns(vrc, depth, pairs):
    """vrc_columns_profile / _fill / _select next to vrc_volume_solid_count, vrc_volume_clone, vrc_volume_fill_boxes and
    vrc_cells_step; see the module's text."""
    import torch
    from cpuvoxelraycaster_amd import scenes
    capi = vrc.capi
    S = 1 << depth
    CALLS = 20                           # a single call is tens of microseconds: a sample times twenty in a row
    res = {"size": S, "pairs": pairs, "calls_per_sample": CALLS, "occupancy_bytes": S ** 3 // 8, "record_bytes": S * S * 16, "map_bytes": S * S * 4}
    records = torch.empty((S * S, 4), dtype=torch.int32, device="cuda")
    lim = np.clip(scenes.terrain_heights(S).astype(np.int64), 16, S)
    hi_map = torch.from_numpy((S // 2 + lim).astype(np.int32)).cuda()
    whole = torch.tensor([0, 0, 0, S, S, S], dtype=torch.int32).cuda()
    torch.cuda.synchronize()

    def case(src):
        dst, other, work = vrc.VoxelVolume(depth), vrc.VoxelVolume(depth), vrc.VoxelVolume(depth)
        one = {"solid_voxels": src.solidCount()}
        for axis, name in enumerate("xyz"):
            e = one["profile_" + name] = {}
            e["ms"], e["solid_count_ms"], e["clone_ms"] = timed_ab([lambda: src.columnProfileDevice(2 * axis, records.data_ptr()), src.solidCount, src.clone], pairs, CALLS)
            e["profile_over_solid_count"] = round(e["ms"]["median"] / e["solid_count_ms"]["median"], 3)
            e["profile_over_clone"] = round(e["ms"]["median"] / e["clone_ms"]["median"], 3)
        e = one["raise_terrain"] = {}
        e["ms"], e["fill_boxes_ms"] = timed_ab([lambda: work.fillColumnsDevice(1, None, S // 2 + 1, hi_map.data_ptr(), 0, None, capi.VRC_COPY_REPLACE) and None,
                                                lambda: other.fillBoxesDevice(1, whole.data_ptr(), True)], pairs, CALLS)
        e["fill_over_fill_boxes"] = round(e["ms"]["median"] / e["fill_boxes_ms"]["median"], 3)
        survive = vrc.count_mask(range(1, 7))
        for axis, name in enumerate("xyz"):
            e = one["select_" + name] = {}
            e["ms"], e["cells_step_6_ms"] = timed_ab([lambda: src.selectColumns(2 * axis, 0, 1, capi.VRC_COLUMNS_SOLID, dst) and None,
                                                      lambda: src.cellStepDevice(other, 0, survive, None, 6)], pairs, CALLS)
            e["select_over_cells_step"] = round(e["ms"]["median"] / e["cells_step_6_ms"]["median"], 3)
        one["selected_voxels"] = dst.solidCount()
        for v in (dst, other, work):
            v.close()
        return one

    scene = vrc.LSVO.fromFastNoiseTerrain(depth)
    terrain = vrc.VoxelVolume.fromScene(scene)
    res["terrain"] = case(terrain)
    raised = vrc.VoxelVolume(depth).fillColumnsDevice(1, None, S // 2 + 1, hi_map.data_ptr(), 0, None, capi.VRC_COPY_REPLACE)
    res["raise_terrain_is_the_scene"] = bool(raised.diff(terrain).stats.words == 0)
    for thing in (raised, terrain, scene):
        thing.close()
    noise = vrc.VoxelVolume(depth).fillRandom(1337, 0.5, None, capi.VRC_COPY_REPLACE)
    res["random_0.5"] = case(noise)
    noise.close()
    return res


class Mode(collections.namedtuple("Mode", "name flag help bench depths writes")):
    """One mode of the tool.  depths: what runs when --depths is not given; writes: the result also goes to
    profiles/edit/bench_<name>.json (the line of the others is put there by hand, see profiles/README.md)."""

    @property
    def label(self):
        return "edit_" + self.name if self.flag else "edit"

    @property
    def file(self):
        return "bench_%s.json" % self.name


# in order of precedence: the first mode whose flag is given runs, the last one without any
MODES = [
    Mode("columns", "--columns", "time vrc_columns_profile / _fill / _select next to vrc_volume_solid_count, vrc_volume_clone, vrc_volume_fill_boxes and vrc_cells_step", bench_columns, [9], True),
    Mode("pack", "--pack", "time vrc_pack_volume / vrc_unpack_volume next to vrc_volume_clone and vrc_volume_download", bench_pack, [9], True),
    Mode("cells", "--cells", "time vrc_cells_step / vrc_cells_fill_random next to vrc_volume_copy_region and vrc_volume_clone", bench_cells, [9], True),
    Mode("delta", "--delta", "time vrc_delta_diff / vrc_delta_apply next to vrc_volume_clone and a copy of one occupancy", bench_delta, [9], True),
    Mode("fracture", "--fracture", "time vrc_fracture_label next to vrc_volume_distance_field + vrc_volume_label_components", bench_fracture, [9], True),
    Mode("clearance", "--clearance", "time vrc_rigid_clearance next to vrc_rigid_contacts with the same maps and boxes", bench_clearance, [9], True),
    Mode("pair_contacts", "--pair-contacts", "time vrc_rigid_box_pairs and vrc_rigid_pair_contacts next to placement + contacts per pair", bench_pair_contacts, [9], True),
    Mode("contacts", "--contacts", "time vrc_rigid_contacts next to vrc_rigid_place_affine with the same maps and boxes", bench_contacts, [9], True),
    Mode("rigid", "--rigid", "time vrc_rigid_moments / vrc_rigid_place_affine next to vrc_labels_select / vrc_fall_place", bench_rigid, [9], True),
    Mode("fall", "--fall", "time vrc_fall_drops / vrc_fall_place next to vrc_volume_label_components of the same debris", bench_fall, [9], True),
    Mode("travel", "--travel", "time vrc_travel_field next to vrc_volume_flood from the same seeds", bench_travel, [9], True),
    Mode("rects", "--rects", "time vrc_rect_count / vrc_extract_rects next to the surface calls", bench_rects, [9], True),
    Mode("stamp", "--stamp", "time vrc_volume_stamp_affine next to vrc_volume_copy_region", bench_stamp, [9], True),
    Mode("distance", "--distance", "time vrc_volume_distance_field / vrc_distance_select / dilate", bench_distance, [9], True),
    Mode("components", "--components", "time vrc_volume_label_components / vrc_labels_*", bench_components, [9], True),
    Mode("surface", "--surface", "time vrc_volume_surface_count / vrc_volume_extract_surface", bench_surface, [9], False),
    Mode("voxelize", "--voxelize", "time vrc_volume_xor_mesh", bench_voxelize, [9], False),
    Mode("flood", "--flood", "time vrc_volume_flood", bench_flood, [9], False),
    Mode("brushes", "--brushes", "time the brushes, copies and queries", bench_brushes, [9, 10], False),
    Mode("edit", None, None, bench_depth, [8, 9, 10], False),
]


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depths", type=int, nargs="+")
    ap.add_argument("--pairs", type=int, default=5)
    for mode in MODES:
        if mode.flag:
            default = ("depth %d" if len(mode.depths) == 1 else "depths %d and %d") % tuple(mode.depths)
            ap.add_argument(mode.flag, action="store_true", help="%s (%s unless --depths is given)" % (mode.help, default))
    return ap


def select(args):
    """(the first mode of MODES whose flag is given, else the last; --depths, else that mode's own)"""
    mode = next(m for m in MODES if not m.flag or getattr(args, m.flag[2:].replace("-", "_")))
    return mode, list(mode.depths) if args.depths is None else args.depths


def run(mode, depths, pairs, vrc, device_name, out_dir):
    out = {"bench": mode.label, "device": device_name, "depths": {}}
    for d in depths:
        out["depths"][str(d)] = mode.bench(vrc, d, max(1, pairs))
    print(json.dumps(out))
    if mode.writes:
        with open(os.path.join(out_dir, mode.file), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return out


def main():
    args = make_parser().parse_args()
    mode, depths = select(args)
    import __graft_entry__ as g
    g.build()
    import torch
    import cpuvoxelraycaster_amd as vrc
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit.py needs a GPU (the library has no CPU fallback)")
    run(mode, depths, args.pairs, vrc, torch.cuda.get_device_name(0), os.path.join(ROOT, "profiles", "edit"))


if __name__ == "__main__":
    main()
