"""The sparse tile stream where csrc/vrc_pack.hip leaves the regime of tests/test_gpu_volume_pack.py, against pack_model.py bit
for bit.  The three volumes are tests/pack_cases.py's, held to their conditions without a GPU in tests/test_pack_cases_host.py:
  strided_512    10.9 million partial bricks: k_unpack_bytes, the file's one grid-stride loop (4096 groups of 256), takes three
                 trips, the last of them partial, with padding behind it; refusals for bytes only a later trip reaches;
  all_mixed_256  all 4096 tiles mixed with 1 to 512 partial bricks, 500 or more in each of the first 1024: scan_slots carries
                 1024 ranks and 2^19 offsets into its second step; refusals in tiles 1023, 1024, 2500 and 4095;
  sparse_1024    depth 10: 262144 tiles, row_of<true> with six bits a tile axis, 256 scan steps, 1024 groups of k_pack_head.
Each volume is made once for the module from its list of edits; every expected byte is the model's, made from the brick
bytes the same list gives in numpy.

Measured on the MI355X: the 24 tests take about 3.5 s together, 1.5 s of that the set-up of strided_512 (its edits and its
model stream on the host); the slowest calls are test_pack_equals_the_model at 0.48 s (strided_512), 0.33 s (sparse_1024) and
0.15 s (all_mixed_256), everything else 0.10 s or less, next to 0.87 s for the slowest call of test_gpu_volume_large.py in
the same run; none skips."""
import ctypes as C

import numpy as np
import pytest

import pack_cases as cases
import pack_model as model
from volume_support import Stream

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
NAMES = list(cases.CASES)


def info_tuple(info):
    return (info.depth, info.tiles, info.mixed_tiles, info.partial_bricks, info.bytes, info.solid, info.full_tiles, info.reserved)


def model_info(stream):
    h = model.header_of(stream)
    return (h[2], h[3], h[4], h[5], h[6] | (h[7] << 32), h[8] | (h[9] << 32), h[10], 0)


def first_difference(got, want):
    want = np.frombuffer(want, np.uint8)
    if got.size != want.size:
        return "lengths %d and %d" % (got.size, want.size)
    at = np.flatnonzero(got != want)
    return "%d bytes differ, the first at %s" % (len(at), at[:4].tolist())


class Held:
    """volume: the case on the device; scratch: what its first pack call added to editScratchBytes(); other: a volume of the
    same depth for the unpacks to overwrite"""


def held(name):
    import cpuvoxelraycaster_amd as vrc
    case = cases.CASES[name]()
    h = Held()
    h.case = case
    h.volume = cases.upload(vrc.VoxelVolume(case.depth), case.edits)
    before = h.volume.editScratchBytes()
    h.sized = h.volume.packInfo()
    h.scratch_before, h.scratch = before, h.volume.editScratchBytes() - before
    h.other = vrc.VoxelVolume(case.depth)
    return h


@pytest.fixture(scope="module")
def volumes(built):
    made = {}

    def get(name):
        if name not in made:
            made[name] = held(name)
        return made[name]

    yield get
    for h in made.values():
        h.volume.close()
        h.other.close()


@pytest.fixture(scope="module")
def dense():
    """dense_of(bricks) of the two cases small enough for a download, made once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = model.dense_of(cases.CASES[name]().bricks)
        return made[name]

    return get


# ---- every case: pack ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_pack_equals_the_model(volumes, name):
    import torch
    from cpuvoxelraycaster_amd import capi
    h = volumes(name)
    case, volume, want = h.case, h.volume, h.case.stream
    n = len(want)
    assert info_tuple(h.sized) == model_info(want), (name, info_tuple(h.sized), model_info(want))
    assert h.scratch == 8 * (model.Shape(case.depth).NT + 1) + 64, (name, h.scratch)
    assert volume.solidCount() == case.solid
    got = volume.pack()
    assert got.tobytes() == want, (name, "host stream", first_difference(got, want))
    dev = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = capi.PackInfo()
    rc = capi.load().vrc_pack_volume(volume._h, capi.ptr(dev.data_ptr()), n, C.byref(info), capi.VRC_MEM_DEVICE)
    got = dev.cpu().numpy()
    assert rc == 0 and info_tuple(info) == model_info(want), (name, info_tuple(info))
    assert got[:n].tobytes() == want, (name, "device stream", first_difference(got[:n], want))
    assert (got[n:] == SENTINEL).all(), (name, "beyond the stream")
    assert volume.editScratchBytes() - h.scratch_before == h.scratch, (name, "the scratch never grows")


# ---- every case: unpack -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("name", NAMES)
def test_unpack_gives_the_volume_back(volumes, dense, name, memory):
    import torch
    h = volumes(name)
    case, target = h.case, h.other
    target.fillRandom(7 if memory == "host" else 8, 0.4, None, 0)           # other content, over everything (0: replace)
    assert target.solidCount() not in (0, case.solid)
    source = case.stream
    if memory == "device":
        source = torch.from_numpy(np.frombuffer(case.stream, np.uint8).copy()).cuda()
        torch.cuda.synchronize()
    target.unpack(source)
    delta = h.volume.diff(target)
    assert delta.count == 0 and int(delta.stats.voxels) == 0, (name, memory, delta.count, int(delta.stats.voxels))
    delta.close()
    assert target.solidCount() == case.solid
    got = target.pack()
    assert got.tobytes() == case.stream, (name, memory, "pack(unpack(s)) == s", first_difference(got, case.stream))
    if case.depth < 10:
        assert np.array_equal(target.download(), dense(name)), (name, memory, "download")
    else:
        places = cases.sparse_places()
        assert target.voxelCount() == case.solid
        assert np.array_equal(target.getVoxels(places.astype(np.uint32)), cases.solid_at(case.bricks, places)), (name, memory, "getVoxels")


# ---- refusals -----------------------------------------------------------------------------------------------------------

def check_refusals(h, target, made):
    """made: [(what, bytes, rule, where)].  Both memory kinds return -1 with the text of the model's (rule, where), and the
    target volume keeps its occupancy"""
    import torch
    from cpuvoxelraycaster_amd import capi
    L = capi.load()
    keep = target.clone()
    for what, bad, rule, where in made:
        text = "vrc_unpack_volume: rule %s" % rule + (" at %s" % where if where else "")
        host = np.frombuffer(bad, np.uint8)
        dev = torch.from_numpy(host.copy()).cuda()
        torch.cuda.synchronize()
        for mem, pointer in ((capi.VRC_MEM_HOST, capi.ptr(host)), (capi.VRC_MEM_DEVICE, capi.ptr(dev.data_ptr()))):
            assert L.vrc_unpack_volume(target._h, pointer, len(bad), mem) == -1, (what, rule, mem)
            assert L.vrc_last_error().decode() == text, (what, mem, L.vrc_last_error().decode(), text)
    delta = keep.diff(target)
    assert delta.count == 0, (made[0][0], "the volume keeps its occupancy", delta.count)
    delta.close()
    keep.close()


@pytest.mark.parametrize("which", cases.A_CORRUPTIONS)
def test_refusals_in_a_later_trip(volumes, which):
    """strided_512's stream with a byte wrong where only the second or third trip of k_unpack_bytes reads it"""
    h = volumes("strided_512")
    bad, rule, where = cases.a_corruption(which)
    check_refusals(h, h.other, [(which, bad, rule, where)])


@pytest.mark.parametrize("rule", cases.B_RULES)
def test_refusals_in_high_tiles(volumes, rule):
    """all_mixed_256's stream with `rule` broken in tiles 1023, 1024, 2500 and 4095, alone and two at a time"""
    h = volumes("all_mixed_256")
    check_refusals(h, h.other, [((rule, tiles), bad, got, where) for tiles, bad, got, where in cases.b_corruptions(rule)])


# ---- ordering -----------------------------------------------------------------------------------------------------------

def test_pack_sees_an_asynchronous_edit_at_512(volumes):
    """a pack right behind a setVoxelsDevice on another stream packs the edited volume"""
    import torch
    h = volumes("strided_512")
    extra, want = cases.ordering_case()
    volume = h.volume.clone()
    t_extra = torch.from_numpy(extra.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with Stream() as stream:
        volume.setVoxelsDevice(len(extra), t_extra.data_ptr(), True, stream)
        got = volume.pack()
    assert got.tobytes() == want, first_difference(got, want)
    volume.close()
