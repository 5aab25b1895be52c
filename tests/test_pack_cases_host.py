"""The cases of tests/test_gpu_volume_pack_large.py without a GPU (tests/pack_cases.py): the restated launch geometry against
a table written by hand, each case held to the regime it is meant for -- on the model's header, never on a device result --,
the brick-wise model against the dense one, and the corruptions against the rule and the place they were made for.  If the
restated geometry stops matching csrc/vrc_pack.hip, update the restatement; the conditions stay."""
import numpy as np

import large_volume_cases
import pack_cases as cases
import pack_model as model


def test_restated_geometry():
    # depth: (pack_tiles, pack_tile_bricks, pack_mask_words, pack_class_words, field_groups, k_unpack_masks' grid, scan steps)
    by_hand = {2: (1, 8, 1, 1, 1, 1, 1), 3: (1, 64, 2, 1, 1, 1, 1), 4: (1, 512, 16, 1, 1, 1, 1), 5: (8, 512, 16, 1, 1, 1, 1),
               6: (64, 512, 16, 4, 1, 4, 1), 7: (512, 512, 16, 32, 2, 32, 1), 8: (4096, 512, 16, 256, 16, 256, 4),
               9: (32768, 512, 16, 2048, 128, 2048, 32), 10: (262144, 512, 16, 16384, 1024, 16384, 256)}
    for depth, row in by_hand.items():
        got = (cases.pack_tiles(depth), cases.pack_tile_bricks(depth), cases.pack_mask_words(depth), cases.pack_class_words(depth),
               cases.field_groups(depth), cases.mask_groups(depth), cases.scan_steps(cases.pack_tiles(depth)))
        assert got == row, (depth, got, row)
        s = model.Shape(depth)
        assert (s.NT, s.K, s.MW, s.CW) == row[:4] and cases.tile_groups(depth) == s.NT
    # P: (words, groups of k_unpack_bytes, trips)
    for P, row in {0: (0, 0, 0), 1: (1, 1, 1), 1024: (256, 1, 1), 1025: (257, 2, 1), 1 << 22: (1 << 20, 4096, 1),
                   (1 << 22) + 1: ((1 << 20) + 1, 4096, 2), 1 << 23: (1 << 21, 4096, 2), (1 << 23) + 5: ((1 << 21) + 2, 4096, 3)}.items():
        assert (cases.byte_words(P), cases.byte_groups(P), cases.byte_trips(P)) == row, P
    assert cases.byte_trip_of(1 << 24, 4 * (1 << 20) - 1) == 0 and cases.byte_trip_of(1 << 24, 4 * (1 << 20)) == 1
    assert cases.tile_number(10, 63, 63, 63) == 262143 and cases.tile_origin(10, 4097).tolist() == [16, 0, 16]
    assert cases.tile_number(8, 9, 12, 4) == 2500 and cases.tile_origin(8, 2500).tolist() == [144, 192, 64]


def test_bricks_of_edits_is_the_dense_path():
    """a list of boxes and voxels, set and cleared, some of them beyond the volume: the bricks of the dense array it makes"""
    rng = np.random.default_rng(3)
    for depth in (3, 5, 6):
        S = 1 << depth
        lo = rng.integers(0, S, (40, 3))
        boxes = np.concatenate([lo, lo + rng.integers(1, S // 2, (40, 3))], axis=1).astype(np.uint32)
        edits = [("boxes", boxes[:25], 1), ("voxels", rng.integers(0, S, (300, 3)).astype(np.uint32), 1), ("boxes", boxes[25:], 0),
                 ("voxels", rng.integers(0, S, (200, 3)).astype(np.uint32), 0), ("boxes", np.array([[1, 0, 3, 4, S, 6]], np.uint32), 1),
                 ("voxels", rng.integers(0, S, (50, 3)).astype(np.uint32), 1)]
        inside = [(kind, np.minimum(items, S) if kind == "boxes" else items, solid) for kind, items, solid in edits]
        dense = large_volume_cases.dense_of(inside, S)
        bricks = cases.bricks_of_edits(edits, depth)
        assert np.array_equal(bricks, model.bricks_of(dense)), depth
        places = rng.integers(-2, S + 2, (500, 3))
        ok = ((places >= 0) & (places < S)).all(1)
        want = np.where(ok, dense[tuple(np.clip(places, 0, S - 1).T)], 0)
        assert np.array_equal(cases.solid_at(bricks, places), want)
        assert np.array_equal(cases.voxels_of(bricks), np.argwhere(dense))


def test_pack_bricks_is_pack():
    for name, field in model.fields(5):
        bricks = model.bricks_of(field)
        stream = model.pack_bricks(bricks, 5)
        assert stream == model.pack(field, 5), name
        assert np.array_equal(model.unpack_bricks(stream, 5), bricks), name
        assert np.array_equal(model.unpack(stream, 5), field), name


def test_strided_512_takes_three_trips():
    case = cases.strided_512()
    P = case.P
    assert case.depth == 9 and P > 1 << 22                                    # lanes of the 4096 x 256 launch take a second word
    assert cases.byte_groups(P) == cases.BYTE_GROUPS and cases.byte_trips(P) == 3
    assert cases.byte_words(P) % (1 << 20) != 0                               # the last trip is partial
    assert P % 4 != 0                                                         # padding exists
    cls = case.classes()
    assert case.full == int((cls == 1).sum()) >= 2 and int((cls == 0).sum()) >= 2 and case.M == int((cls == 2).sum())
    for k in range(1, cases.scan_steps(len(cls))):                            # mixed tiles around every 1024-slot boundary
        assert (cls[1024 * k - 2:1024 * k + 2] == 2).all(), k
    assert len(set(case.partial_counts().tolist())) > 20                      # the counts differ from tile to tile
    assert len(case.stream) < 1 << 24


def test_strided_512_cannot_pass_with_one_trip():
    """the negative control: the byte check cut after the first trip's 2^20 words finds a solid count other than the header's,
    and never comes to the padding; the whole check finds the header's"""
    case = cases.strided_512()
    first_byte, first_padding, solid = cases.byte_check(case.stream)
    assert (first_byte, first_padding) == (None, None) and cases.mask_solid(case.stream) + solid == case.solid
    for words in (1 << 20, 1 << 21):
        _, _, short = cases.byte_check(case.stream, words)
        assert cases.mask_solid(case.stream) + short < case.solid, words


def test_all_mixed_256_has_large_ranks_and_offsets():
    case = cases.all_mixed_256()
    counts = case.partial_counts()
    assert case.depth == 8 and case.M == 4096 == len(counts) and case.full == 0
    assert counts.min() == 1 and counts.max() == 512
    assert np.array_equal(counts, cases.all_mixed_counts())
    assert (counts[:1024] >= 500).all() and int(counts[:1024].sum()) > 1 << 18       # the carry out of the first scan step
    assert int(counts[:1024].sum()) > (1 << 19) - (1 << 13)                          # ... is near 2^19
    assert len(set(counts.tolist())) > 400
    tiles = model.tiles_of(case.bricks, model.Shape(8))
    has_full = (tiles == 0xFF).any(1)
    assert np.array_equal(has_full, counts < 512) and int((counts == 512).sum()) >= 50
    prefix, total = large_volume_cases.scan_slots(counts)
    wrong, _ = large_volume_cases.scan_slots(counts, carry=False)
    assert total == case.P and (wrong[1024:] != prefix[1024:]).all()                 # a lost carry moves every later tile's bytes
    got = model.unpack_bricks(model.pack_bricks(case.bricks, 8), 8)
    assert not isinstance(got, tuple) and np.array_equal(got, case.bricks)


def test_sparse_1024_lies_around_the_step_boundaries():
    case = cases.sparse_1024()
    cls = case.classes()
    assert case.depth == 10 and len(cls) == 262144 and cases.scan_steps(len(cls)) == 256
    both = [k for k in range(1, 256) if cls[1024 * k - 1] == 2 and cls[1024 * k] == 2]
    assert len(both) >= 4 and both[0] == 1 and both[-1] == 255, both
    assert set(cases.C_BOUNDARY_STEPS) <= set(both)
    assert case.full >= 3 and (cls[cases.sparse_listed_tiles()] == 2).all()
    assert cls[0] == cls[1] == cls[262143] == 2
    assert 0 < case.M < 8192 and case.P % 4 != 0
    mixed = np.flatnonzero(cls == 2)
    assert len(set((mixed // 1024).tolist())) > 128                                  # mixed tiles in more than half of the steps
    places = cases.sparse_places()
    want = cases.solid_at(case.bricks, places)
    assert 0 < int(want.sum()) < len(want) and not ((places >= 0) & (places < 1024)).all()
    assert model.solid_of(case.bricks) == case.solid


def test_corruptions_of_strided_512():
    case = cases.strided_512()
    P = case.P
    d, length = model.Shape(9).offsets(case.M, P)[3:]
    at = cases.a_places()
    last = cases.byte_trips(P) - 1
    assert last == 2
    assert [cases.byte_trip_of(P, at[k]) for k in ("trip 1", "trip 1 b", "last", "last b")] == [1, 1, last, last]
    assert all(4 * (1 << 20) <= at[k] < P for k in at) and at["last"] > 4 * (1 << 20) * last
    assert cases.byte_trip_of(P, length - 1 - d) == last
    want = {"zero byte, trip 1": ("partial-byte", "byte %d" % (d + at["trip 1"])),
            "zero byte, last trip": ("partial-byte", "byte %d" % (d + at["last"])),
            "ff byte, trip 1": ("partial-byte", "byte %d" % (d + at["trip 1 b"])),
            "ff byte, last trip": ("partial-byte", "byte %d" % (d + at["last b"])),
            "padding": ("padding", "byte %d" % (length - 1)),
            "solid count": ("solid-count", None),
            "two bytes, trips 1 and 2": ("partial-byte", "byte %d" % (d + at["trip 1"])),       # the lower of the two
            "byte and padding": ("partial-byte", "byte %d" % (d + at["last b"]))}             # the earlier rule
    assert list(want) == cases.A_CORRUPTIONS
    for name in cases.A_CORRUPTIONS:
        bad, rule, where = cases.a_corruption(name)
        assert (rule, where) == want[name], name
        assert len(bad) == len(case.stream) and bad[:d] == case.stream[:d]            # the header and the masks are untouched
        differing = np.flatnonzero(np.frombuffer(bad, np.uint8) != np.frombuffer(case.stream, np.uint8))
        assert 1 <= len(differing) <= 2 and differing[0] >= d + 4 * (1 << 20)         # nothing the first trip reads
    bad = cases.a_corruption("solid count")[0]
    assert cases.byte_check(bad)[:2] == (None, None) and abs(cases.byte_check(bad)[2] - cases.byte_check(case.stream)[2]) == 1


def test_corruptions_of_all_mixed_256():
    case = cases.all_mixed_256()
    assert cases.B_TILES == (1023, 1024, 2500, 4095)
    for rule in cases.B_RULES:
        made = cases.b_corruptions(rule)
        assert [tiles for tiles, _, _, _ in made] == [(t,) for t in cases.B_TILES] + list(cases.B_PAIRS)
        for tiles, bad, got, where in made:
            assert got == rule and len(bad) == len(case.stream) and bad != case.stream, (rule, tiles)
            assert where == (None if rule == "mixed-count" else "tile %d" % min(tiles)), (rule, tiles, where)
