"""The affine stamp on the GPU (vrc_volume_stamp_affine; VoxelVolume.stampAffine / stampPlaced / transformed).  The expected
volume is the numpy model of tests/stamp_model.py (held against the definition in tests/test_volume_stamp_host.py), or
np.transpose / np.flip / vrc_volume_copy_region where a test says so.  Every comparison is np.array_equal on
vrc_volume_download: there are no tolerances."""

import numpy as np
import pytest

import stamp_model as model
from volume_support import Stream, volume_of

pytestmark = pytest.mark.gpu

OPS = (model.REPLACE, model.OR, model.ANDNOT)


def random_volume(rng, depth, density):
    S = 1 << depth
    return (rng.random((S, S, S)) < density).astype(np.uint8)


class Pair:
    """a source and a pre-filled destination on the device with their dense copies; check() stamps into a clone of the
    destination and compares with the model"""

    def __init__(self, seed, src_depth, dst_depth, src_density=0.3, dst_density=0.5):
        rng = np.random.default_rng(seed)
        self.src, self.dst = random_volume(rng, src_depth, src_density), random_volume(rng, dst_depth, dst_density)
        self.d_src, self.d_dst = volume_of(self.src, src_depth), volume_of(self.dst, dst_depth)
        self.S = 1 << dst_depth

    def check(self, m, t, lo=None, hi=None, ops=OPS, what=None):
        import cpuvoxelraycaster_amd as vrc
        results = []
        for op in ops:
            work = self.d_dst.clone()
            work.stampAffine(self.d_src, vrc.make_affine(m, t), lo, hi, op)
            got = work.download()
            work.close()
            want = model.stamp(self.dst, self.src, m, t, lo, hi, op)
            assert np.array_equal(got, want), (what, m, t, lo, hi, op, int((got != want).sum()))
            results.append(want)
        return results

    def close(self):
        self.d_src.close()
        self.d_dst.close()


def odd_boxes(S):
    """the whole volume, odd bounds on every axis, one voxel, a box clipped by the volume, an empty and an inverted one"""
    return [(None, None), ((1, 3, 1), (S - 1, S - 2, S - 1)), ((S // 2 + 1, 1, S - 3), (S // 2 + 2, 2, S - 2)), ((0, 1, 3), (S + 9, S, 0xFFFFFFFF)),
            ((1, 1, 1), (1, S, S)), ((3, 0, 0), (2, S, S))]


# ---- small volumes: two rows to a word ------------------------------------------------------------------------------

@pytest.mark.parametrize("src_depth", [2, 3])
def test_depth_2_destination_takes_atomics(built, src_depth):
    """4^3: one occupancy word holds two brick rows, so the rows' threads share it and take 32-bit vector atomics.  All three
    ops into a randomly pre-filled destination, every kind of box."""
    pair = Pair(700 + src_depth, src_depth, 2)
    Ss = 1 << src_depth
    rng = np.random.default_rng(70 + src_depth)
    maps = [model.IDENTITY, model.signed_permutation((1, 0, 2), (0, 1, 0), Ss), model.signed_permutation((2, 0, 1), (1, 1, 0), Ss),
            ([model.ONE * Ss // 4, 0, 0, 0, model.ONE * Ss // 4, 0, 0, 0, model.ONE * Ss // 4], [0, 0, 0])] + model.aimed_maps(rng, Ss, 4, 6)
    changed = 0
    for m, t in maps:
        for lo, hi in odd_boxes(4):
            want = pair.check(m, t, lo, hi, what="depth 2")
            changed += int(not np.array_equal(want[0], pair.dst))
    assert changed >= 10
    pair.close()


@pytest.mark.parametrize("src_depth,dst_depth", [(3, 3), (2, 3), (5, 5), (3, 5)])
def test_plain_store_sizes(built, src_depth, dst_depth):
    """depth 3 (n = 4: the first size where a word has one owner and is written with a plain store) and depth 5, with every
    kind of box"""
    pair = Pair(800 + 10 * src_depth + dst_depth, src_depth, dst_depth)
    Ss, Sd = 1 << src_depth, 1 << dst_depth
    rng = np.random.default_rng(80 + src_depth + dst_depth)
    k = model.ONE * Ss // Sd
    maps = [([k, 0, 0, 0, k, 0, 0, 0, k], [0, 0, 0]), model.signed_permutation((0, 2, 1), (0, 0, 1), Ss)] + model.aimed_maps(rng, Ss, Sd, 3)
    for m, t in maps:
        for lo, hi in odd_boxes(Sd):
            pair.check(m, t, lo, hi, what="plain stores")
    pair.close()


def test_empty_boxes_touch_nothing(built):
    pair = Pair(5, 3, 4)
    for lo, hi in [((0, 0, 0), (0, 0, 0)), ((5, 5, 5), (5, 9, 9)), ((9, 0, 0), (3, 16, 16)), ((16, 0, 0), (20, 16, 16)), ((0, 0, 16), (16, 16, 0xFFFFFFFF))]:
        for want in pair.check(*model.IDENTITY, lo, hi, what="empty box"):
            assert np.array_equal(want, pair.dst)
    pair.close()


# ---- the 48 turns and mirrorings ------------------------------------------------------------------------------------

def test_signed_permutations_at_8(built):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 3, 8
    rng = np.random.default_rng(48)
    src = random_volume(rng, depth, 0.3)
    d_src = volume_of(src, depth)
    images = set()
    for perm, flip in model.all_signed_permutations():
        turned = d_src.transformed(vrc.affine_signed_permutation(perm, flip, S))
        got = turned.download()
        turned.close()
        assert np.array_equal(got, model.permuted(src, perm, flip)), (perm, flip)
        assert np.array_equal(got, model.stamp(np.zeros_like(src), src, *model.signed_permutation(perm, flip, S)))
        images.add(got.tobytes())
    assert len(images) == 48
    d_src.close()


def test_quarter_turn_and_back_restores_the_volume(built):
    import cpuvoxelraycaster_amd as vrc
    depth, S = 5, 32
    src = random_volume(np.random.default_rng(90), depth, 0.3)
    d_src = volume_of(src, depth)
    turned = d_src.transformed(vrc.affine_signed_permutation((1, 0, 2), (0, 1, 0), S))
    p = np.indices((S, S, S))
    assert np.array_equal(turned.download(), src[p[1], S - 1 - p[0], p[2]])
    restored = turned.transformed(vrc.affine_signed_permutation((1, 0, 2), (1, 0, 0), S))
    assert np.array_equal(restored.download(), src)
    for v in (restored, turned, d_src):
        v.close()


def test_identity_equals_copy_region(built):
    import cpuvoxelraycaster_amd as vrc
    pair = Pair(32, 5, 5)
    lo, hi = (3, 1, 5), (30, 27, 32)
    size = tuple(h - l for l, h in zip(lo, hi))
    for op in OPS:
        stamped, copied = pair.d_dst.clone(), pair.d_dst.clone()
        stamped.stampAffine(pair.d_src, vrc.make_affine(*model.IDENTITY), lo, hi, op)
        copied.copyRegion(pair.d_src, lo, size, lo, op)
        got = stamped.download()
        assert np.array_equal(got, copied.download()), op
        assert np.array_equal(got, model.stamp(pair.dst, pair.src, *model.IDENTITY, lo, hi, op))
        stamped.close()
        copied.close()
    pair.close()


# ---- random and extreme maps ----------------------------------------------------------------------------------------

def test_random_maps(built):
    """Source density 0.3.  Rotations from affine_place, shears, negative and zero rows, the all-zero matrix, the scales, the
    limits, and maps that miss the source altogether."""
    import cpuvoxelraycaster_amd as vrc
    depth, S = 5, 32
    pair = Pair(1234, depth, depth)
    rng = np.random.default_rng(4321)
    box = ((1, 0, 3), (S - 1, S - 3, S))
    ONE = model.ONE

    # rotations: about each axis, about two, with a scale and pivots off the lattice
    turns = [model.rotation(2, np.radians(30)), model.rotation(0, 1.0), model.rotation(1, -2.2),
             model.compose(model.rotation(0, np.radians(30)), model.rotation(1, np.radians(30))), model.compose(model.rotation(2, 0.8), model.rotation(0, 2.9))]
    for i, rot in enumerate(turns):
        scale = (1.0, 0.7, 1.3, 1.0, 2.5)[i]
        a, lo, hi = vrc.affine_place(rot, scale, (16.0, 15.5, 16.25), (16.0 + i, 16.0, 14.5), depth, depth)
        want = pair.check(list(a.m), list(a.t), lo, hi, what="rotation")
        assert not np.array_equal(want[0], pair.dst)
        pair.check(list(a.m), list(a.t), what="rotation, whole volume")
    # shears, negative rows, zero rows
    shear = [ONE, ONE // 2, 0, 0, ONE, -ONE // 3, ONE // 5, 0, ONE]
    for m, t in [(shear, [0, 3 << 17, -(2 << 17)]),
                 ([-ONE, 0, 0, 0, -ONE, 0, 0, 0, -ONE], [S << 17] * 3),
                 ([-ONE, -ONE, -ONE, ONE, 0, 0, 0, ONE, 0], [(3 * S // 2) << 18, 0, 0]),
                 ([0, 0, 0, 0, ONE, 0, 0, 0, ONE], [5 << 17, 0, 0]),
                 ([ONE, 0, 0, 0, 0, 0, 0, 0, 0], [0, (7 << 17) + 9, 31 << 17]),
                 ([0, 0, 0, 0, 0, 0, 0, 0, -ONE], [1, 2, S << 17])]:
        pair.check(m, t, *box, what="shear / negative / zero rows")
    # the all-zero matrix: every voxel reads the one source voxel at t >> 17
    solid, hole = np.argwhere(pair.src)[5], np.argwhere(pair.src == 0)[5]
    for at, bit in [(solid, 1), (hole, 0)]:
        t = [(int(v) << 17) + 12345 for v in at]
        want = pair.check([0] * 9, t, *box, what="zero matrix")
        inside = want[0][box[0][0]:box[1][0], box[0][1]:box[1][1], box[0][2]:box[1][2]]
        assert (inside == bit).all()
    pair.check([0] * 9, [-1, 0, 0], *box, what="zero matrix, outside")
    # scales 1/16, 1/3, 1/2, 2, 3 and 16 (m = ONE / scale): the source seen 16, 3 and 2 times smaller, 2, 3 and 16 times
    # larger.  ONE // 3 = 21845 is the inexact entry: the 17-bit fraction carries unevenly along a word's 8 z steps
    for k in (16 * ONE, 3 * ONE, 2 * ONE, ONE // 2, ONE // 3, ONE // 16):
        for t in ([0, 0, 0], [-(40 << 17) + 77, 1 << 16, (3 << 17) - 1]):
            pair.check([k, 0, 0, 0, k, 0, 0, 0, k], t, what=("scale", k))
    # m and t at their limits
    big, far = model.M_LIMIT, model.T_LIMIT
    for m, t in [([big] * 9, [-far] * 3), ([-big] * 9, [far] * 3), ([big, -big, big, -big, big, big, big, big, -big], [far, -far, far]),
                 ([big, 0, 0, 0, big, 0, 0, 0, big], [-(big * 2 * 20) + (9 << 17)] * 3),          # crosses the source around voxel 10
                 ([-big, 0, 0, 0, big, 0, 0, 0, -big], [big * 2 * 30, -(big * 2 * 8), big * 2 * 41])]:
        pair.check(m, t, what="limits")
    # the whole box outside the source: REPLACE clears the box, OR and ANDNOT leave dst untouched
    for m, t in [(model.IDENTITY[0], [S << 17, 0, 0]), (model.IDENTITY[0], [0, -(S << 17), 0]), (model.IDENTITY[0], [0, 0, far]), ([big] * 9, [far] * 3)]:
        replaced, ored, carved = pair.check(m, t, *box, what="outside")
        cleared = pair.dst.copy()
        cleared[box[0][0]:box[1][0], box[0][1]:box[1][1], box[0][2]:box[1][2]] = 0
        assert np.array_equal(replaced, cleared) and np.array_equal(ored, pair.dst) and np.array_equal(carved, pair.dst)
    # and a batch of general matrices
    for m, t in model.aimed_maps(rng, S, S, 12):
        pair.check(m, t, *box, ops=(int(rng.integers(0, 3)),), what="general")
    pair.close()


@pytest.mark.parametrize("src_depth,dst_depth", [(4, 6), (6, 4)])
def test_depths_differ(built, src_depth, dst_depth):
    import cpuvoxelraycaster_amd as vrc
    pair = Pair(60 + src_depth, src_depth, dst_depth, dst_density=0.1)
    Ss, Sd = 1 << src_depth, 1 << dst_depth
    k = model.ONE * Ss // Sd
    pair.check([k, 0, 0, 0, k, 0, 0, 0, k], [0, 0, 0], what="fit")
    pair.check(*model.IDENTITY, what="identity")
    pair.check(model.IDENTITY[0], [-(5 << 17), 3 << 17, -(1 << 17)], (1, 1, 1), (Sd - 1, Sd - 1, Sd - 1), what="shifted")
    rot = model.compose(model.rotation(2, 0.6), model.rotation(1, -0.4))
    a, lo, hi = vrc.affine_place(rot, 1.0 * Sd / Ss / 2, (Ss / 2,) * 3, (Sd / 2 + 1.5, Sd / 2, Sd / 2), src_depth, dst_depth)
    pair.check(list(a.m), list(a.t), lo, hi, what="placed")
    for m, t in model.aimed_maps(np.random.default_rng(6), Ss, Sd, 4):
        pair.check(m, t, what="general")
    pair.close()


# ---- ordering -------------------------------------------------------------------------------------------------------

def test_stream_order_behind_device_memory_edits(built):
    """an asynchronous fill_boxes on src and one on dst, then the stamp, all on one created stream with no host
    synchronisation in between: the stamp sees both"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    depth, S = 5, 32
    pair = Pair(77, depth, depth, dst_density=0.05)
    src_boxes = np.array([[2, 3, 4, 20, 9, 30], [25, 25, 0, 31, 32, 7]], np.uint32)
    dst_boxes = np.array([[0, 0, 0, 32, 4, 32], [10, 10, 10, 13, 29, 11]], np.uint32)
    d_src_boxes = torch.from_numpy(src_boxes.view(np.int32).copy()).cuda()
    d_dst_boxes = torch.from_numpy(dst_boxes.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    m, t = model.signed_permutation((2, 0, 1), (0, 1, 1), S)
    lo, hi = (1, 2, 3), (31, 32, 29)
    with Stream() as stream:
        pair.d_src.fillBoxesDevice(2, d_src_boxes.data_ptr(), True, stream)
        pair.d_dst.fillBoxesDevice(2, d_dst_boxes.data_ptr(), True, stream)
        pair.d_dst.stampAffine(pair.d_src, vrc.make_affine(m, t), lo, hi, model.ANDNOT, stream)
    src, dst = pair.src.copy(), pair.dst.copy()
    for b in src_boxes:
        src[b[0]:b[3], b[1]:b[4], b[2]:b[5]] = 1
    for b in dst_boxes:
        dst[b[0]:b[3], b[1]:b[4], b[2]:b[5]] = 1
    want = model.stamp(dst, src, m, t, lo, hi, model.ANDNOT)
    assert not np.array_equal(want, model.stamp(pair.dst, pair.src, m, t, lo, hi, model.ANDNOT))         # the edits matter
    assert np.array_equal(pair.d_dst.download(), want)
    pair.close()


def test_stamp_then_commit(built):
    """commit waits for the stamp, whatever its stream: the committed scene's nodes are vrc_scene_build_volume's of the
    model's result"""
    import cpuvoxelraycaster_amd as vrc
    depth = 5
    pair = Pair(88, depth, depth, dst_density=0.02)
    rot = model.compose(model.rotation(0, np.radians(30)), model.rotation(2, np.radians(30)))
    a, lo, hi = vrc.affine_place(rot, 0.75, (16.0,) * 3, (15.0, 16.0, 17.0), depth, depth)
    scratch = (pair.d_dst.editScratchBytes(), pair.d_src.editScratchBytes())
    with Stream() as stream:
        pair.d_dst.stampAffine(pair.d_src, a, lo, hi, model.OR, stream)
        svo = pair.d_dst.commit()
    want = model.stamp(pair.dst, pair.src, list(a.m), list(a.t), lo, hi, model.OR)
    ref = vrc.LSVO.fromVolume(want, depth)
    got_nodes, want_nodes = svo.downloadNodes(), ref.downloadNodes()
    assert got_nodes.shape == want_nodes.shape and np.array_equal(got_nodes.view(np.uint64), want_nodes.view(np.uint64))
    assert not np.array_equal(want, pair.dst)
    assert (pair.d_dst.editScratchBytes(), pair.d_src.editScratchBytes()) == scratch       # the stamp allocates no scratch
    for v in (svo, ref):
        v.close()
    pair.close()


# ---- the Python conveniences ----------------------------------------------------------------------------------------

def test_stamp_placed_and_transformed(built):
    import cpuvoxelraycaster_amd as vrc
    rng = np.random.default_rng(99)
    clip_depth, world_depth = 4, 6
    clip, world = random_volume(rng, clip_depth, 0.3), random_volume(rng, world_depth, 0.02)
    d_clip, d_world = volume_of(clip, clip_depth), volume_of(world, world_depth)
    rot = model.compose(model.rotation(1, np.radians(30)), model.rotation(0, np.radians(30)))
    # defaults: about the two centres, OR
    a, lo, hi = d_world.stampPlaced(d_clip, rot, 2.0)
    assert (list(a.m), list(a.t), list(lo), list(hi)) == tuple(model.place(rot, 2.0, (8.0,) * 3, (32.0,) * 3, clip_depth, world_depth))
    want = model.stamp(world, clip, list(a.m), list(a.t), lo, hi, model.OR)
    assert np.array_equal(d_world.download(), want) and int(want.sum()) > int(world.sum()) + 4 * int(clip.sum())
    # pivots and op given: carve the same model out again somewhere else
    a, lo, hi = d_world.stampPlaced(d_clip, rot, 1.25, (0.0, 8.0, 16.0), (50.5, 12.0, 30.0), vrc.capi.VRC_COPY_ANDNOT)
    want = model.stamp(want, clip, list(a.m), list(a.t), lo, hi, model.ANDNOT)
    assert np.array_equal(d_world.download(), want)
    # transformed: the same depth by default, another on request
    flipped = d_clip.transformed(vrc.affine_signed_permutation((0, 1, 2), (0, 0, 1), 16))
    assert flipped.depth == clip_depth and np.array_equal(flipped.download(), clip[:, :, ::-1])
    doubled = d_clip.transformed(vrc.make_affine([32768, 0, 0, 0, 32768, 0, 0, 0, 32768], [0, 0, 0]), depth=5)
    assert doubled.depth == 5 and np.array_equal(doubled.download(), clip.repeat(2, 0).repeat(2, 1).repeat(2, 2))
    assert np.array_equal(d_clip.download(), clip)
    for v in (doubled, flipped, d_world, d_clip):
        v.close()
