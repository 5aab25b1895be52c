"""The numpy model of the volume deltas (include/vrc.h: vrc_delta_diff, vrc_delta_apply): the yardstick of
test_volume_delta_host.py and test_gpu_volume_delta.py.  Occupancy is dense [x, y, z] uint8 on one side and the uint32 word
array of the key rule on the other: key = 8 B + (z&1) 4 + (y&1) 2 + (x&1) with B = ((x>>1) n + (y>>1)) n + (z>>1), n = S / 2,
word = key >> 5, bit = key & 31."""
import numpy as np

RECORD_DTYPE = np.dtype([("word", "<u4"), ("bits", "<u4")])


def words_of(dense):
    """the uint32 word array (8^depth / 32 words) of an [x, y, z] occupancy"""
    S = dense.shape[0]
    n = S // 2
    cells = (np.asarray(dense) != 0).reshape(n, 2, n, 2, n, 2).transpose(0, 2, 4, 5, 3, 1)     # cx cy cz | zb yb xb
    weights = (1 << np.arange(8, dtype=np.uint32)).reshape(2, 2, 2)                            # bit zb*4 + yb*2 + xb
    bricks = (cells * weights).sum(axis=(3, 4, 5)).astype(np.uint8)                            # byte B = (cx n + cy) n + cz
    return np.ascontiguousarray(bricks).reshape(-1).view("<u4").copy()


def dense_of(words, depth):
    """the [x, y, z] uint8 occupancy of a word array"""
    n = 1 << (depth - 1)
    bricks = np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(n, n, n)
    bits = (bricks[..., None] >> np.arange(8, dtype=np.uint8)) & 1                             # cx cy cz | bit
    cells = bits.reshape(n, n, n, 2, 2, 2).transpose(0, 5, 1, 4, 2, 3)                         # cx xb cy yb cz zb
    return np.ascontiguousarray(cells).reshape(2 * n, 2 * n, 2 * n).astype(np.uint8)


def diff(a, b, depth):
    """(records, stats) of the word arrays a = before and b = after: stats = dict(words, voxels, lo, hi), hi exclusive,
    lo = hi = (0, 0, 0) for an empty delta"""
    x = np.asarray(a, np.uint32) ^ np.asarray(b, np.uint32)
    W = np.flatnonzero(x)
    records = np.zeros(len(W), RECORD_DTYPE)
    records["word"], records["bits"] = W, x[W]
    changed = dense_of(x, depth)
    lo, hi = [0, 0, 0], [0, 0, 0]
    if len(W):
        for axis in range(3):
            along = np.flatnonzero(changed.any(axis=tuple(k for k in range(3) if k != axis)))
            lo[axis], hi[axis] = int(along[0]), int(along[-1]) + 1
    return records, dict(words=len(W), voxels=int(changed.sum(dtype=np.uint64)), lo=tuple(lo), hi=tuple(hi))


def apply(words, records):
    """a new word array: words[word] ^= bits for every record"""
    out = np.array(words, np.uint32)
    out[records["word"]] ^= records["bits"]
    return out


def stats_tuple(stats):
    """a capi.DeltaStats (or the model's dict) as (words, voxels, lo, hi, reserved)"""
    if isinstance(stats, dict):
        return (stats["words"], stats["voxels"], tuple(stats["lo"]), tuple(stats["hi"]), (0, 0))
    return (int(stats.words), int(stats.voxels), tuple(stats.lo), tuple(stats.hi), tuple(stats.reserved))
