"""The calls between depths without a GPU: every refusal that precedes a device call by its whole text, the symbols and the
wrappers, count_range, the numpy model (levels_model.py) against itself, and the C++ adapter's new methods."""
import ctypes as C
import os

import numpy as np
import pytest

import levels_model as model
from volume_support import ROOT, check_cpp_syntax


def handle(fill=0, **words):
    """512 bytes that stand for a handle: every 32-bit word `fill`, then words[index] = value"""
    block = (C.c_uint32 * 128)(*([fill] * 128))
    for name, value in words.items():
        block[int(name[1:])] = value
    return block


# `device` is the first 32-bit word of a vrc_volume and `depth` its third
ZERO, DEPTH_3, ALSO_3, DEPTH_5, DEVICE_1 = handle(), handle(w2=3), handle(w2=3), handle(w2=5), handle(w0=1, w2=5)
COUNTS = (C.c_uint32 * 8)(*([0x55] * 8))


def p(a):
    return None if a is None else C.cast(a, C.c_void_p)


def counts_args(src=DEPTH_3, k=1, counts=COUNTS, mem=0):
    return (p(src), k, p(counts), mem, None)


def reduce_args(dst=DEPTH_3, src=DEPTH_5, lo=1, hi=9, op=0):
    return (p(dst), p(src), lo, hi, op, None)


def expand_args(dst=DEPTH_5, src=DEPTH_3, op=0):
    return (p(dst), p(src), op, None)


# every refusal of the vrc_levels_* entry points, all before the first HIP call: the WHOLE vrc_last_error() text, as literals
REFUSALS = [
    ("vrc_levels_counts", counts_args(src=None), "null volume"),
    ("vrc_levels_counts", counts_args(counts=None), "null counts"),
    ("vrc_levels_counts", counts_args(k=0), "k 0 not in [1, 3], the volume's depth"),
    ("vrc_levels_counts", counts_args(k=4), "k 4 not in [1, 3], the volume's depth"),
    ("vrc_levels_counts", counts_args(src=DEPTH_5, k=0xFFFFFFFF), "k 4294967295 not in [1, 5], the volume's depth"),
    ("vrc_levels_counts", counts_args(src=ZERO, k=1), "k 1 not in [1, 0], the volume's depth"),
    ("vrc_levels_counts", counts_args(mem=2), "bad mem kind 2"),
    ("vrc_levels_counts", counts_args(k=3, mem=-1), "bad mem kind -1"),
    ("vrc_levels_reduce", reduce_args(dst=None), "null argument"),
    ("vrc_levels_reduce", reduce_args(src=None), "null argument"),
    ("vrc_levels_reduce", reduce_args(dst=DEPTH_5), "source and destination are the same volume"),
    ("vrc_levels_reduce", reduce_args(src=DEVICE_1), "volumes on devices 0 and 1"),
    ("vrc_levels_reduce", reduce_args(dst=DEVICE_1, src=DEPTH_5), "volumes on devices 1 and 0"),
    ("vrc_levels_reduce", reduce_args(src=ALSO_3), "destination of depth 3 is not below the source's 3"),
    ("vrc_levels_reduce", reduce_args(dst=DEPTH_5, src=DEPTH_3), "destination of depth 5 is not below the source's 3"),
    ("vrc_levels_reduce", reduce_args(dst=DEPTH_3, src=ZERO), "destination of depth 3 is not below the source's 0"),
    ("vrc_levels_reduce", reduce_args(op=3), "bad op 3"),
    ("vrc_levels_reduce", reduce_args(op=-1), "bad op -1"),
    ("vrc_levels_expand", expand_args(dst=None), "null argument"),
    ("vrc_levels_expand", expand_args(src=None), "null argument"),
    ("vrc_levels_expand", expand_args(src=DEPTH_5), "source and destination are the same volume"),
    ("vrc_levels_expand", expand_args(dst=DEVICE_1), "volumes on devices 1 and 0"),
    ("vrc_levels_expand", expand_args(dst=ALSO_3), "destination of depth 3 is not above the source's 3"),
    ("vrc_levels_expand", expand_args(dst=DEPTH_3, src=DEPTH_5), "destination of depth 3 is not above the source's 5"),
    ("vrc_levels_expand", expand_args(dst=ZERO), "destination of depth 0 is not above the source's 3"),
    ("vrc_levels_expand", expand_args(op=3), "bad op 3"),
    ("vrc_levels_expand", expand_args(op=-2), "bad op -2"),
    # two refusals at once: the one that wins
    ("vrc_levels_reduce", reduce_args(dst=DEPTH_5, op=3), "source and destination are the same volume"),
    ("vrc_levels_reduce", reduce_args(dst=DEVICE_1, src=DEPTH_3), "volumes on devices 1 and 0"),
    ("vrc_levels_reduce", reduce_args(src=DEVICE_1, op=3), "volumes on devices 0 and 1"),
    ("vrc_levels_reduce", reduce_args(src=ALSO_3, op=-1), "destination of depth 3 is not below the source's 3"),
    ("vrc_levels_expand", expand_args(src=DEPTH_5, op=3), "source and destination are the same volume"),
    ("vrc_levels_expand", expand_args(dst=DEVICE_1, src=DEPTH_5), "volumes on devices 1 and 0"),
    ("vrc_levels_expand", expand_args(dst=DEVICE_1, op=3), "volumes on devices 1 and 0"),
    ("vrc_levels_expand", expand_args(dst=ALSO_3, op=3), "destination of depth 3 is not above the source's 3"),
]


def untouched():
    return (not any(ZERO) and list(DEPTH_3) == [0, 0, 3] + [0] * 125 == list(ALSO_3) and list(DEPTH_5) == [0, 0, 5] + [0] * 125
            and list(DEVICE_1) == [1, 0, 5] + [0] * 125 and list(COUNTS) == [0x55] * 8)


@pytest.mark.parametrize("index", range(len(REFUSALS)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(REFUSALS)])
def test_levels_refusal_text(built, index):
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    name, args, text = REFUSALS[index]
    assert getattr(L, name)(*args) == -1                                     # VRC_ERR_INVALID
    assert L.vrc_last_error() == ("%s: %s" % (name, text)).encode()
    assert untouched()                                                       # nothing was written through any handle or buffer


def test_every_levels_entry_point_has_its_refusals():
    from cpuvoxelraycaster_amd import capi
    names = {n for n in capi.SYMBOLS if n.startswith("vrc_levels_")}
    assert names == {"vrc_levels_counts", "vrc_levels_reduce", "vrc_levels_expand"} == {c[0] for c in REFUSALS}
    assert not any(n.startswith("vrc_volume_") for n in names)


def test_wrappers_and_exports():
    import cpuvoxelraycaster_amd as vrc
    for name in ("cellCounts", "cellCountsDevice", "reduceInto", "expandInto", "reduced", "expanded", "levels", "countRange"):
        assert callable(getattr(vrc.VoxelVolume, name)), name
    assert "count_range" in vrc.__all__ and vrc.VoxelVolume.countRange is vrc.count_range


def test_count_range_names_the_four_rules():
    import cpuvoxelraycaster_amd as vrc
    for k in range(1, 9):
        full = 8 ** k
        assert vrc.count_range("any", k) == (1, full + 1) == model.count_range("any", k)
        assert vrc.count_range("all", k) == (full, full + 1) == model.count_range("all", k)
        assert vrc.count_range("majority", k) == (full // 2, full + 1) == model.count_range("majority", k)
        assert vrc.count_range("empty", k) == (0, 1) == model.count_range("empty", k)
        assert vrc.count_range((3, 7), k) == (3, 7) == model.count_range((3, 7), k)
        assert vrc.count_range(np.array([2, 5], np.uint32), k) == (2, 5)
    with pytest.raises(ValueError):
        vrc.count_range("most", 2)


@pytest.mark.parametrize("S", [8, 16, 32])
def test_model_counts_pool_and_sum(S):
    rng = np.random.default_rng(700 + S)
    vol = (rng.random((S, S, S)) < 0.5).astype(np.uint8)
    depth = S.bit_length() - 1
    below = vol.astype(np.uint32)
    for k in range(1, depth + 1):
        c = model.counts(vol, k)
        Sc = S >> k
        assert c.shape == (Sc, Sc, Sc) and c.dtype == np.uint32 and int(c.sum()) == int(vol.sum())
        assert np.array_equal(c, below.reshape(Sc, 2, Sc, 2, Sc, 2).sum((1, 3, 5)))          # the 2 x 2 x 2 sum-pool of level k - 1
        below = c
    assert model.counts(vol, depth).tolist() == [[[int(vol.sum())]]]


def test_model_reduce_and_expand_by_hand():
    vol = np.zeros((8, 8, 8), np.uint8)
    vol[0:2, 0:2, 0:2] = 1                                 # cell (0, 0, 0) of level 1: full
    vol[7, 7, 6] = 1                                       # cell (3, 3, 3): one voxel
    vol[2:4, 4:6, 0] = 1                                   # cell (1, 2, 0): four voxels, half
    any_, all_, half = (model.reduced(vol, 2, rule) for rule in ("any", "all", "majority"))
    assert sorted(map(tuple, np.argwhere(any_).tolist())) == [(0, 0, 0), (1, 2, 0), (3, 3, 3)]
    assert np.argwhere(all_).tolist() == [[0, 0, 0]] and sorted(map(tuple, np.argwhere(half).tolist())) == [(0, 0, 0), (1, 2, 0)]
    assert model.reduced(vol, 2, "empty").sum() == 64 - 3 and model.reduced(vol, 2, (5, 5)).sum() == 0
    ones = np.ones((4, 4, 4), np.uint8)
    assert np.array_equal(model.reduce(ones, vol, 1, 9, model.ANDNOT), 1 - any_) and np.array_equal(model.reduce(all_, vol, 4, 5, model.OR), half)
    big = model.expand(np.zeros((8, 8, 8), np.uint8), any_)
    assert big.sum() == 3 * 8 and big[6:8, 6:8, 6:8].all() and big[2:4, 4:6, 0:2].all()
    for rule in ("any", "all"):
        assert np.array_equal(model.reduced(big, 2, rule), any_)
    assert np.array_equal(model.expand(np.ones((8, 8, 8), np.uint8), any_, model.ANDNOT), 1 - big)


def test_host_adapter_with_levels_compiles(built):
    """HipVoxelVolume::cellCounts / reduceInto / reduced / expandInto / expanded in the header-only adapter: C++14, no HIP headers"""
    hdr = os.path.join(ROOT, "cpuvoxelraycaster_amd", "host", "hip_raycaster.hpp")
    src = ('#include "%s"\n'
           'uint64_t use(vrc_host::HipVoxelVolume& world, vrc_host::HipVoxelVolume& coarse) {\n'
           '    using Rule = vrc_host::HipVoxelVolume::LevelRule;\n'
           '    const std::vector<uint32_t> density = world.cellCounts(3);\n'
           '    uint32_t lo, hi;\n'
           '    vrc_host::HipVoxelVolume::countRange(Rule::Majority, 2, &lo, &hi);\n'
           '    world.reduceInto(coarse, lo, hi);\n'
           '    world.reduceInto(coarse, 1, 9, VRC_COPY_ANDNOT);\n'
           '    coarse.expandInto(world, VRC_COPY_OR);\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> proxy = world.reduced(4), inner = world.reduced(4, Rule::All);\n'
           '    std::unique_ptr<vrc_host::HipVoxelVolume> sketch = coarse.expanded(world.depth());\n'
           '    return density.size() + lo + hi + proxy->depth() + inner->depth() + sketch->depth();\n'
           '}\n'
           'int main() { return 0; }\n') % hdr
    check_cpp_syntax(src, strict=True)
