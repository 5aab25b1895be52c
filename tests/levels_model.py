"""The numpy model of the calls between depths (include/vrc.h: vrc_levels_counts, vrc_levels_reduce, vrc_levels_expand): the
yardstick of test_levels_host.py, test_gpu_volume_levels.py and test_gpu_volume_levels_cpp.py.  Occupancy is dense [x, y, z]
uint8, counts are uint32 [X, Y, Z]."""
import numpy as np

from cells_model import ANDNOT, OR, REPLACE, apply_op  # noqa: F401

RULES = ("any", "all", "majority", "empty")


def counts(vol, k):
    """the solid voxels of every cube of 2^k voxels per axis"""
    S = vol.shape[0]
    f = 1 << k
    Sc = S // f
    return (np.asarray(vol) != 0).reshape(Sc, f, Sc, f, Sc, f).sum((1, 3, 5)).astype(np.uint32)


def count_range(rule, k):
    full = 8 ** k
    if isinstance(rule, str):
        return {"any": (1, full + 1), "all": (full, full + 1), "majority": (full // 2, full + 1), "empty": (0, 1)}[rule]
    return int(rule[0]), int(rule[1])


def reduce(dst, vol, lo, hi, op=REPLACE):
    """a copy of dst after vrc_levels_reduce from vol"""
    k = (vol.shape[0] // dst.shape[0]).bit_length() - 1
    c = counts(vol, k).astype(np.int64)
    K = ((c >= lo) & (c < hi)).astype(np.uint8)
    return apply_op(dst.astype(np.uint8), K, op)


def reduced(vol, depth, rule="any"):
    S = 1 << depth
    k = (vol.shape[0] // S).bit_length() - 1
    return reduce(np.zeros((S, S, S), np.uint8), vol, *count_range(rule, k))


def expand(dst, vol, op=REPLACE):
    """a copy of dst after vrc_levels_expand from vol"""
    f = dst.shape[0] // vol.shape[0]
    E = np.repeat(np.repeat(np.repeat((np.asarray(vol) != 0).astype(np.uint8), f, 0), f, 1), f, 2)
    return apply_op(dst.astype(np.uint8), E, op)
