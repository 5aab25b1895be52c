"""The cases of tests/test_gpu_volume_rects_long.py without a GPU (tests/rect_cases.py): the word-by-word emulation of
csrc/vrc_rects.hip's count, scan and emit equals the numpy model (rect_model.rects) on every scene up to 128^3 and on random
fields at depths 2 to 6; the plane-by-plane sparse model equals the dense one; the records that follow from how the sheets
are made are the model's; every scene takes the word walks it was made for (counted by the emulation, the counts stated
here); and the ten wrong kernels, emulated, change the record lists of the scenes by the pinned numbers.

Nine of the ten are caught.  Number 8, rect_starts without pcarry, cannot be caught by any scene: pcarry only clears bit 0
of "the row before starts a run at this bit", a mask whose one use is to let a start skip the exact test (holds_run).
Without it fewer starts skip the test and the test decides the same, so the records are the same and only the work grows.
The test pins that: no record changes, and holds_run is called more often.

These are conditions on the cases, not measurements of the kernels.  If the restated geometry stops matching the code,
update the restatement; the conditions stay."""
import functools

import numpy as np
import pytest

import rect_cases as K
import rect_model as R


@functools.lru_cache(maxsize=None)
def fields_of(scene):
    return K.row_fields(scene.dense())


def emulation(scene, wrong=0, closed=True):
    return K.Emulation(fields_of(scene), scene.depth, closed, wrong)


@functools.lru_cache(maxsize=None)
def right(scene, closed=True):
    r = R.rects(scene.dense(), closed)
    r.setflags(write=False)
    return r


def changed(got, want):
    """(records of `got` that `want` lacks, records of `want` that `got` lacks)"""
    a = {tuple(r) for r in np.asarray(got).tolist()}
    b = {tuple(r) for r in np.asarray(want).tolist()}
    return len(a - b), len(b - a)


def run_words(records):
    """the words of its row that each record's run covers"""
    u = R.unpack(records)
    r0 = u[np.arange(len(u)), np.asarray(R.RUN)[u[:, 3] >> 1]]
    return ((r0 + u[:, 4] - 1) >> 5) - (r0 >> 5) + 1


# ---- a. the restated geometry ------------------------------------------------------------------------------------------

def test_restated_geometry():
    assert [K.words_lg(d) for d in (2, 4, 5, 6, 7, 8, 9, 10)] == [0, 0, 0, 1, 2, 3, 4, 5]
    assert [K.field_words(d) for d in (2, 4, 5, 6, 7, 9)] == [16, 256, 1024, 8192, 65536, 1 << 22]
    assert [K.groups_of(d) for d in (2, 3, 4, 5, 6, 7, 8, 9, 10)] == [1, 2, 6, 24, 192, 1536, 12288, 98304, 786432]
    # depth 4 is the first at which a workgroup lies inside one direction (256 lanes = one direction's S^2 words) ..
    assert K.field_words(4) == K.GROUP and K.field_words(3) < K.GROUP
    # .. and depths 7, 8, 9 need 2, 12 and 96 steps of the scan
    assert [K.scan_steps(K.groups_of(d)) for d in (6, 7, 8, 9)] == [1, 2, 12, 96] and K.SCAN_GROUP == 1024
    for depth in (2, 4, 5, 6, 7, 9):
        S, w = 1 << depth, 1 << K.words_lg(depth)
        rng = np.random.default_rng(depth)
        for d, ca, cs, k in zip(rng.integers(0, 6, 50), rng.integers(0, S, 50), rng.integers(0, S, 50), rng.integers(0, w, 50)):
            L = K.lane_index(int(d), int(ca), int(cs), int(k), depth)
            assert L == ((d * S + ca) * S + cs) * w + k < K.lanes_of(depth) and K.lane_parts(L, depth) == (d, ca, cs, k)


@pytest.mark.parametrize("depth", [3, 5, 6])
def test_row_fields_and_face_words(depth):
    """the two row fields hold the voxels bit for bit, and face_word by the kernel's indices is the rule of the model"""
    S, w = 1 << depth, max(1, (1 << depth) // 32)
    V = (np.random.default_rng(40 + depth).random((S, S, S)) < 0.6).astype(np.uint8)
    fields = K.row_fields(V)
    assert fields.dtype == np.uint32 and fields.shape == (2 * K.field_words(depth),)
    x, y, z = np.indices((S, S, S))
    assert np.array_equal((fields[(x * S + y) * w + (z >> 5)] >> (z & 31)) & 1, V)
    assert np.array_equal((fields[K.field_words(depth) + (x * S + z) * w + (y >> 5)] >> (y & 31)) & 1, V)
    for closed in (True, False):
        table = K.face_words(fields, depth, closed)
        mask = R.face_masks(V, closed)
        for d in range(6):
            a = d >> 1
            M = mask[d].transpose(a, R.STACK[a], R.RUN[a])
            ca, cs, cr = np.indices((S, S, S))
            assert np.array_equal(((table[d][ca, cs, cr >> 5] >> (cr & 31).astype(np.uint32)) & 1).astype(bool), M), (d, closed)
        rng = np.random.default_rng(depth)
        for d, ca, cs, k in zip(rng.integers(0, 6, 200), rng.integers(0, S, 200), rng.integers(0, S, 200), rng.integers(0, w, 200)):
            assert K.face_word(fields, depth, 0 if closed else K.M32, int(d), int(ca), int(cs), int(k)) == int(table[d, ca, cs, k])


# ---- b. the emulation is the model -------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_emulation_on_random_fields(depth):
    S = 1 << depth
    for density in (0.5, 0.9)[:1 if depth == 6 else 2]:
        V = (np.random.default_rng(10 * depth + int(10 * density)).random((S, S, S)) < density).astype(np.uint8)
        for closed in (True, False):
            want = R.rects(V, closed)
            assert np.array_equal(K.emulated(V, closed), want), (depth, density, closed)
            assert np.array_equal(K.sparse_rects(K.DensePlanes(V), closed), want), (depth, density, closed)


def test_emulation_at_depth_4():
    S = 16
    board = (np.indices((S, S, S)).sum(axis=0) & 1).astype(np.uint8)
    for V in (K.small_constructed(S), board, np.ones((S, S, S), np.uint8), np.zeros((S, S, S), np.uint8)):
        for closed in (True, False):
            assert np.array_equal(K.emulated(V, closed), R.rects(V, closed))
    up = R.unpack(R.rects(K.small_constructed(S), False))
    up = up[(up[:, 3] == 3) & (up[:, 1] == 7)]
    assert up.tolist() == K.SMALL_UP


def scenes_128():
    return [K.pair_table(7, a) for a in range(3)] + [K.stacks(7, a) for a in range(3)] + [K.blocky(7, 2), K.blocky(7, 1), K.full_volume(7)] + \
           [K.slab(7, a, s) for a in range(3) for s in (0, 1)]


# per scene of the pair tables and stacks: what the emulation counted, closed.  [run_end calls by further words 0, 1, 2, 3+],
# holds_run's middle-word visits and the calls decided false there, reads of bit 31 of word k0 - 1 and how many decided,
# reads of bit 0 of word k1 + 1 and how many decided, calls with r1 == S
PATHS = {
    "pairs x 128": ([2852, 1829, 1374, 735], 864, 216, 108, 26, 252, 196, 510),
    "pairs y 128": ([3736, 1771, 1374, 735], 864, 216, 108, 26, 252, 196, 510),
    "pairs z 128": ([75980, 1196, 976, 512], 864, 216, 108, 26, 252, 196, 340),
    "stacks x 128": ([14, 6, 272, 280], 1560, 4, 512, 0, 0, 0, 524),
    "stacks y 128": ([539, 6, 272, 276], 1560, 4, 512, 0, 0, 0, 520),
    "stacks z 128": ([1702, 6, 268, 268], 1560, 4, 512, 0, 0, 0, 516),
}


@pytest.mark.parametrize("index", range(15))
def test_scenes_at_128(index):
    scene = scenes_128()[index]
    for closed in (True, False):
        want = right(scene, closed)
        em = emulation(scene, 0, closed)
        assert np.array_equal(em.records(), want), (scene.name, closed)
        assert np.array_equal(K.sparse_rects(scene.planes(), closed), want), (scene.name, closed)
        if scene.axis is not None:
            # sheets at inner planes: what follows from the construction, closed or open
            assert np.array_equal(K.sheet_records(want, scene.axis), scene.expected), (scene.name, closed)
        elif scene.expected is not None:
            assert np.array_equal(want, scene.expected if closed else scene.expected[:0]), (scene.name, closed)
        if closed and scene.name in PATHS:
            got = (em.loops, em.middle_visits, em.middle_false, em.low_reads, em.low_false, em.high_reads, em.high_false, em.row_end_calls)
            print(scene.name, got)
            assert got == PATHS[scene.name]
            # what the scene is for: run_end's loop twice and more, a middle word visited and deciding, both aligned-edge
            # reads (the stacks are word-aligned at the low end only), r1 == S at a word edge
            assert em.loops[2] > 0 and em.loops[3] > 0 and em.middle_visits > 0 and em.middle_false > 0 and em.low_reads > 0 and em.row_end_calls > 0
            if scene.name.startswith("pairs"):
                assert em.low_false > 0 and em.high_reads > 0 and em.high_false > 0
    # the scan takes a second step, with records on both sides of its edge
    group = K.lane_of(right(scene), scene.S) // K.GROUP
    assert K.groups_of(7) > K.SCAN_GROUP and (group < K.SCAN_GROUP).any()
    if "slab" not in scene.name:
        assert (group >= K.SCAN_GROUP).any()


def test_pair_table_holds_every_pair():
    """every r0 with every r1 at least two cells on, in every variant; the holes in every word of the run, middle words too"""
    S = 128
    assert K.pair_starts(S) == [0, 1, 31, 32, 33, 63, 64]
    assert K.pair_ends(S) == [31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
    for axis in range(3):
        assert K.pair_table(7, axis).pairs == 520
    variants = K.pair_variants(S, 1, 128)
    assert [v[0] for v in variants[:5]] == ["same", "short-lo", "short-hi", "long-lo"] + ["hole"]          # r1 = S: no longer one at the high end
    assert [runs[0][1] for what, runs in variants if what == "hole"] == [15, 31, 32, 47, 63, 64, 79, 95, 96, 111]
    assert ("long-hi", [(0, 97)]) in K.pair_variants(S, 0, 96) and ("long-lo", [(31, 96)]) in K.pair_variants(S, 32, 96)


@pytest.mark.parametrize("run_axis", [2, 1])
def test_blocky_fields_hold_long_runs_in_bulk(run_axis):
    """counted on the field alone.  Runs over three or more words (the rows of every rectangle whose run does): 3754 along z,
    1882 along y.  Merge decisions settled in a middle word, by the emulation: 652 and 347"""
    scene = K.blocky(7, run_axis)
    want = right(scene)
    u = R.unpack(want)
    long_runs = int(u[run_words(want) >= 3, 5].sum())
    em = emulation(scene)
    assert np.array_equal(em.records(), want)
    print(scene.name, long_runs, em.middle_false, em.loops, em.low_reads, em.low_false, em.high_reads, em.high_false)
    assert (long_runs, em.middle_false) == {2: (3754, 652), 1: (1882, 347)}[run_axis]
    assert long_runs >= 1000 and em.middle_false >= 100
    assert em.loops[2] > 0 and em.loops[3] > 0 and em.low_false > 0 and em.high_false > 0 and em.row_end_calls > 0


# ---- the wrong kernels -------------------------------------------------------------------------------------------------

def switch_scenes():
    return [K.pair_table(7, a) for a in range(3)] + [K.stacks(7, a) for a in range(3)] + [K.blocky(7, 2)]


# wrong kernel: {scene: (records it gives that are not the model's, records of the model it lacks)}; a scene not named keeps
# its records
CHANGED = {
    1: {"pairs x 128": (2844, 2758), "pairs y 128": (2825, 2739), "pairs z 128": (1880, 1794), "stacks x 128": (552, 36), "stacks y 128": (548, 32),
        "stacks z 128": (536, 20), "blocky z 128": (20669, 9446)},
    2: {"pairs x 128": (1518, 1476), "pairs y 128": (1518, 1476), "pairs z 128": (1008, 966), "stacks x 128": (548, 32), "stacks y 128": (544, 28),
        "stacks z 128": (532, 16), "blocky z 128": (3754, 1890)},
    3: {"pairs x 128": (216, 216), "pairs y 128": (216, 216), "pairs z 128": (216, 216), "stacks x 128": (2, 4), "stacks y 128": (2, 4),
        "stacks z 128": (2, 4), "blocky z 128": (28, 55)},
    4: {"pairs x 128": (26, 26), "pairs y 128": (26, 26), "pairs z 128": (26, 26), "blocky z 128": (13, 13)},
    5: {"pairs x 128": (28, 196), "pairs y 128": (28, 196), "pairs z 128": (28, 196), "blocky z 128": (15, 34)},
    6: {"pairs x 128": (2, 0), "blocky z 128": (1259, 554)},      # the next row in memory is the next stack row only on the x faces
    7: {"pairs x 128": (4862, 0), "pairs y 128": (4843, 0), "pairs z 128": (3220, 0), "stacks x 128": (1380, 0), "stacks y 128": (1368, 0),
        "stacks z 128": (1336, 0), "blocky z 128": (24992, 0)},
    8: {},
    9: {"pairs z 128": (1245, 1245), "stacks x 128": (10, 10), "stacks y 128": (18, 18), "stacks z 128": (30, 30), "blocky z 128": (2122, 2122)},
    10: {"pairs x 128": (0, 4210), "pairs y 128": (0, 4210), "pairs z 128": (0, 3500), "stacks x 128": (0, 35), "stacks y 128": (0, 35),
         "stacks z 128": (0, 30), "blocky z 128": (0, 13174)},
}


@pytest.mark.parametrize("wrong", range(1, 11))
def test_wrong_kernels_change_the_records(wrong):
    found, work = {}, [0, 0]
    for scene in switch_scenes():
        em = emulation(scene, wrong)
        c = changed(em.records(), right(scene))
        if c != (0, 0):
            found[scene.name] = c
        assert wrong != 8 or em.holds_calls >= emulation_calls(scene), scene.name
        work[0] += em.holds_calls
        work[1] += emulation_calls(scene)
    print(wrong, K.WRONG[wrong], found)
    assert found == CHANGED[wrong]
    assert bool(found) == (wrong != 8)
    if wrong == 8:
        assert work == [239983, 239437]                                     # the same records for more calls of holds_run


@functools.lru_cache(maxsize=None)
def emulation_calls(scene):
    em = emulation(scene)
    em.records()
    return em.holds_calls


# ---- the sparse scenes of 256^3 and 512^3 ------------------------------------------------------------------------------

def test_pair_starts_and_ends_reach_every_word_of_a_long_row():
    for S in (256, 512):
        assert K.pair_starts(S) == [0, 1, 31, 32, 33, 63, 64, S // 2 - 1, S // 2, S // 2 + 1, S - 32]
        assert K.pair_ends(S) == sorted([e - 1 for e in range(32, S + 1, 32)] + list(range(32, S + 1, 32)) + [e + 1 for e in range(32, S, 32)])
    words = {(k, p) for what, runs in K.pair_variants(512, 1, 512) if what == "hole" for k, p in [divmod(runs[0][1], 32)]}
    assert words == {(0, 15), (0, 31), (1, 0), (1, 15), (1, 31), (7, 0), (7, 15), (7, 31), (15, 0), (15, 15)}


@pytest.mark.parametrize("depth,axis", [(8, 0), (8, 1), (8, 2), (9, 0), (9, 1), (9, 2)])
def test_sparse_pair_tables(depth, axis):
    """the sparse model gives what the construction says; at 256^3 the emulation on the dense field gives the same and walks
    middle words; the records lie on both sides of the first step of the scan"""
    scene = K.pair_table(depth, axis)
    S = scene.S
    assert len(scene.boxes) < 1 << 16 and (scene.pairs - 1) // (S // 3) * 2 + 1 < S - 1
    want = K.sparse_rects(scene.planes(), True)
    assert np.array_equal(K.sheet_records(want, axis), scene.expected)
    assert np.array_equal(R.ordered(want), want)
    assert run_words(scene.expected).max() == S // 32
    group = K.lane_of(want, S) // K.GROUP
    assert K.groups_of(depth) > K.SCAN_GROUP and (group < K.SCAN_GROUP).any() and (group >= K.SCAN_GROUP).any()
    if depth == 8:
        em = emulation(scene)
        assert np.array_equal(em.records(), want)
        assert em.loops[3] > 0 and em.middle_false > 0 and em.low_false > 0 and em.high_false > 0 and em.row_end_calls > 0
        em.wrong = 10                                                       # the same starts under the wrong scan
        assert changed(em.records(), want)[1] > 0


@pytest.mark.parametrize("depth", [8, 9])
def test_sparse_stacks_full_volume_and_slabs(depth):
    S = 1 << depth
    for axis in range(3):
        scene = K.stacks(depth, axis)
        for closed in (True, False):
            want = K.sparse_rects(scene.planes(), closed)
            assert np.array_equal(K.sheet_records(want, axis), scene.expected)
            if depth == 8:
                assert np.array_equal(emulation(scene, 0, closed).records(), want)
    full = K.full_volume(depth)
    assert np.array_equal(K.sparse_rects(full.planes(), True), full.expected) and K.sparse_rects(full.planes(), False).shape == (0, 4)
    assert R.unpack(full.expected)[:, 4:].tolist() == [[S, S]] * 6
    for axis in range(3):
        for side in (0, 1):
            scene = K.slab(depth, axis, side)
            u = R.unpack(K.sparse_rects(scene.planes(), True))
            assert u.shape[0] == 6 and sorted(u[:, 3].tolist()) == list(range(6))
            # the four thin faces: rows along z (or y) one high where the slab is thin along their stack axis, S rows of one cell
            # where it is thin along their run axis
            assert sorted(u[:, 4:].tolist()) == [[1, S]] * (0, 2, 4)[axis] + [[S, 1]] * (4, 2, 0)[axis] + [[S, S]] * 2
            u = R.unpack(K.sparse_rects(scene.planes(), False))
            assert u.tolist() == [[0 if a != axis else (S - 1 if side else 0) for a in range(3)] + [2 * axis + (1 - side), S, S]]
