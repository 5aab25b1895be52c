"""The sparse tile stream on the device (include/vrc.h: vrc_pack_volume, vrc_unpack_volume) against the numpy model of
pack_model.py, bit for bit: streams, infos, refusals and every download.  A tile takes one slot in each of the two slot
arrays (csrc/vrc_pack.hip), so 256^3 with its 4096 tiles is the first size at which the slot scan takes a second step (four
there)."""
import ctypes as C

import numpy as np
import pytest

import pack_model as model
from volume_support import Stream, committed, expected_nodes, same, terrain_volume, volume_of

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def info_tuple(info):
    return (info.depth, info.tiles, info.mixed_tiles, info.partial_bricks, info.bytes, info.solid, info.full_tiles, info.reserved)


def model_info(stream):
    h = model.header_of(stream)
    return (h[2], h[3], h[4], h[5], h[6] | (h[7] << 32), h[8] | (h[9] << 32), h[10], 0)


def pack_call(volume, buf, capacity, mem):
    """(rc, info) of vrc_pack_volume into buf (a numpy array, a device pointer or None)"""
    from cpuvoxelraycaster_amd import capi
    info = capi.PackInfo()
    rc = capi.load().vrc_pack_volume(volume._h, capi.ptr(buf), capacity, C.byref(info), mem)
    return rc, info


def check_field(field, depth, what, other=None, nodes=True):
    """everything the issue lists for one field: pack against the model, the size-only call, capacities, both memory kinds,
    unpack into a volume that holds `other`, pack(unpack(s)) == s, and the commit of the unpacked volume"""
    import torch
    from cpuvoxelraycaster_amd import capi
    want = model.pack(field, depth)
    n = len(want)
    volume = volume_of(field, depth)
    before = volume.editScratchBytes()
    rc, sized = pack_call(volume, None, 0, capi.VRC_MEM_HOST)
    assert rc == 0 and info_tuple(sized) == model_info(want), (what, info_tuple(sized), model_info(want))
    assert sized.solid == volume.solidCount() == int(field.sum())
    scratch = volume.editScratchBytes() - before
    assert scratch == 8 * (model.Shape(depth).NT + 1) + 64, (what, scratch)
    # host memory: exact capacity with a sentinel behind it, then a short capacity
    host = np.full(n + 16, SENTINEL, np.uint8)
    rc, info = pack_call(volume, host, n, capi.VRC_MEM_HOST)
    assert rc == 0 and info_tuple(info) == info_tuple(sized), what
    assert host[:n].tobytes() == want, (what, "host stream", np.flatnonzero(host[:n] != np.frombuffer(want, np.uint8))[:4])
    assert (host[n:] == SENTINEL).all(), (what, "beyond the stream")
    host[:] = SENTINEL
    rc, info = pack_call(volume, host, n - 1, capi.VRC_MEM_HOST)
    assert rc == -1 and info_tuple(info) == info_tuple(sized) and (host == SENTINEL).all(), (what, "short capacity")
    assert capi.load().vrc_last_error().decode() == "vrc_pack_volume: capacity %d below the stream's %d bytes" % (n - 1, n)
    # device memory, the same two
    dev = torch.full((n + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, info = pack_call(volume, dev.data_ptr(), n - 4, capi.VRC_MEM_DEVICE)
    assert rc == -1 and info_tuple(info) == info_tuple(sized) and bool((dev == SENTINEL).all()), (what, "short device capacity")
    rc, info = pack_call(volume, dev.data_ptr(), n, capi.VRC_MEM_DEVICE)
    got = dev.cpu().numpy()
    assert rc == 0 and got[:n].tobytes() == want and (got[n:] == SENTINEL).all(), (what, "device stream")
    assert volume.pack().tobytes() == want and volume.pack(device=True).cpu().numpy().tobytes() == want
    assert volume.editScratchBytes() - before == scratch, (what, "the scratch never grows")
    # unpack into a volume holding another field, from host and from device memory
    if other is None:
        other = (np.random.default_rng(5).random(field.shape) < 0.3).astype(np.uint8)
    for source in (want, dev[:n]):
        target = volume_of(other, depth)
        target.unpack(source)
        assert np.array_equal(target.download(), field), (what, "unpack", type(source).__name__)
        assert target.pack().tobytes() == want, (what, "pack(unpack(s)) == s")
        if nodes and source is want:
            assert same(committed(target), expected_nodes(field, depth)), (what, "commit of the unpacked volume")
        target.close()
    volume.close()
    return want


@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6])
def test_fields_against_the_model(built, depth):
    for name, field in model.fields(depth):
        check_field(field, depth, (depth, name))


@pytest.mark.parametrize("depth", [2, 3, 5, 6])
def test_refusals_name_the_rule_and_keep_the_volume(built, depth):
    import torch
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    fields = dict(model.fields(depth))
    held = fields["random 0.50"]
    volume = volume_of(held, depth)
    tried = set()
    for name in ("random 0.02", "P % 4 = 3", "tile-aligned box", "sphere", "empty"):      # empty: at one tile the only stream with a class-0 tile
        stream = model.pack(fields[name], depth)
        cases = [(rule, bad, where) for rule, _, bad, where in model.corruptions(stream)]
        for cut in model.boundaries(stream):                  # truncated (or run on) 4 bytes either side of every section boundary
            for n_bytes in (cut - 4, cut + 4):
                if n_bytes != len(stream):
                    cases.append(("header-short" if n_bytes < 64 else "length-argument", (stream + bytes(4))[:n_bytes], None))
        for rule, bad, where in cases:
            assert model.unpack(bad, depth) == (rule, where), (depth, name, rule)
            text = "vrc_unpack_volume: rule %s" % rule + (" at %s" % where if where else "")
            host = np.frombuffer(bad, np.uint8)
            dev = torch.from_numpy(host.copy()).cuda()
            torch.cuda.synchronize()
            for mem, pointer in ((capi.VRC_MEM_HOST, capi.ptr(host)), (capi.VRC_MEM_DEVICE, capi.ptr(dev.data_ptr()))):
                assert L.vrc_unpack_volume(volume._h, pointer, len(bad), mem) == -1, (depth, name, rule, mem)
                assert L.vrc_last_error().decode() == text, (depth, name, rule, mem, L.vrc_last_error().decode(), text)
            tried.add(rule)
        assert np.array_equal(volume.download(), held), (depth, name, "the volume keeps its occupancy")
    assert tried == set(model.RULES) - (set() if depth == 2 else {"mask-range"}), set(model.RULES) - tried
    # a stream of another depth
    import cpuvoxelraycaster_amd as vrc
    other_depth = depth + 1 if depth < 6 else 5
    with pytest.raises(vrc.VrcError, match="vrc_unpack_volume: rule depth"):
        volume.unpack(model.pack(np.ones((1 << other_depth,) * 3, np.uint8), other_depth))
    assert np.array_equal(volume.download(), held)
    volume.close()


def test_terrain_at_128(built, heights):
    field = terrain_volume(heights, 7)
    stream = check_field(field, 7, "terrain 128^3")
    assert len(stream) < field.size // 8                       # smaller than the occupancy it stands for


def test_scan_carries_at_256(built):
    """256^3 has 4096 tiles and a tile one slot per array, so scan_slots takes four steps of 1024: mixed tiles on both sides
    of every 1024-slot boundary with partial counts that all differ, so a lost carry shifts ranks and bytes"""
    S, T = 256, 16
    field = np.zeros((S, S, S), np.uint8)
    field[:16, :16, :16] = 1                                  # tile 0 full
    tiles = [1, 2, 1022, 1023, 1024, 1025, 2046, 2047, 2048, 2049, 3071, 3072, 3073, 4094, 4095]
    for k, t in enumerate(tiles):
        tx, ty, tz = t // (T * T), (t // T) % T, t % T
        block = field[16 * tx:16 * tx + 16, 16 * ty:16 * ty + 16, 16 * tz:16 * tz + 16]
        block[:8, :8, :8] = 1                                 # whole bricks ...
        for i in range(3 * k + 1):                            # ... and 3 k + 1 partial ones
            block[8 + 2 * (i % 4), 2 * ((i // 4) % 8), 15 - 2 * (i // 32)] = 1
    want = model.pack(field, 8)
    h = model.header_of(want)
    assert h[4] == len(tiles) and h[5] == sum(3 * k + 1 for k in range(len(tiles))) and h[10] == 1
    other = np.zeros((S, S, S), np.uint8)
    other[::2, 1::2, ::3] = 1
    check_field(field, 8, "256^3", other=other, nodes=False)


def test_misaligned_device_buffers_are_refused(built):
    import torch
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    field = dict(model.fields(5))["sphere"]
    volume = volume_of(field, 5)
    stream = model.pack(field, 5)
    n = len(stream)
    dev = torch.full((n + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for shift in (1, 2, 3):
        rc, _ = pack_call(volume, dev.data_ptr() + shift, n, capi.VRC_MEM_DEVICE)
        assert rc == -1 and L.vrc_last_error().decode().endswith("is not aligned to 4 bytes")
        assert bool((dev == SENTINEL).all())
    dev[4:4 + n] = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    target = volume_of(np.zeros_like(field), 5)
    assert L.vrc_unpack_volume(target._h, capi.ptr(dev.data_ptr() + 4), n, capi.VRC_MEM_DEVICE) == 0
    assert np.array_equal(target.download(), field)
    dev[5:5 + n] = dev[4:4 + n].clone()
    torch.cuda.synchronize()
    target.fillBoxes([[0, 0, 0, 3, 3, 3]])
    held = target.download()
    assert L.vrc_unpack_volume(target._h, capi.ptr(dev.data_ptr() + 5), n, capi.VRC_MEM_DEVICE) == -1
    assert L.vrc_last_error().decode().endswith("is not aligned to 4 bytes") and np.array_equal(target.download(), held)
    for v in (volume, target):
        v.close()


def test_pack_sees_an_asynchronous_edit(built):
    import torch
    rng = np.random.default_rng(12)
    field = (rng.random((32, 32, 32)) < 0.4).astype(np.uint8)
    extra = rng.integers(0, 32, (6000, 3)).astype(np.uint32)
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    torch.cuda.synchronize()
    edited = field.copy()
    edited[tuple(extra.astype(np.int64).T)] = 1
    volume = volume_of(field, 5)
    with Stream() as stream:
        volume.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
        got = volume.pack()
    assert got.tobytes() == model.pack(edited, 5)
    # ... and an unpack right behind such an edit replaces what the edit wrote
    with Stream() as stream:
        volume.setVoxelsDevice(len(extra), t_extra.data_ptr(), False, stream)
        volume.unpack(model.pack(field, 5))
    assert np.array_equal(volume.download(), field)
    volume.close()


def test_from_packed_and_files(built, tmp_path):
    import cpuvoxelraycaster_amd as vrc
    field = dict(model.fields(6))["sphere"]
    volume = volume_of(field, 6)
    path = str(tmp_path / "world.vrcp")
    info = volume.save(path)
    want = model.pack(field, 6)
    assert open(path, "rb").read() == want and info.bytes == len(want)
    for made in (vrc.VoxelVolume.load(path), vrc.VoxelVolume.fromPacked(want), vrc.VoxelVolume.fromPacked(volume.pack(device=True))):
        assert made.depth == 6 and np.array_equal(made.download(), field)
        made.close()
    with pytest.raises(vrc.VrcError, match="vrc_pack_header: rule length-argument"):
        vrc.VoxelVolume.fromPacked(want[:-4])
    volume.close()
