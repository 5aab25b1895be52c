"""Every row of the table "Ordering of the volume's entry points"  held on the device, one case per record of
tests/ordering_cases.py, direction and memory form.

Waits for: on a stream A the ballast, then a device-memory vrc_volume_set_voxels of the subject the row names; on a second
vrc_stream_create stream B (the NULL stream for the NULL-stream rows) the call under test, with no synchronisation; its result
and every subject's content are the models' of the state AFTER the edit, exactly.  The rows with two roles get each late
alone and both late together on two ballast streams.  Recorded as an edit of: the call itself in device form on A behind the
ballast, then vrc_volume_download on the NULL stream with no synchronisation: it shows the call's result.  One row has no
such case: vrc_volume_flood is recorded as an edit of region, but it returns only when its work is done (the sweeps read a
flag back), so no reader can come too early whether the record is made or not -- a test cannot observe that record, and none
here claims to.  The three extractors run twice back to back with different windows, the first behind the ballast on A, the
second on B: both lists are the model's, and when B is done A is done too -- the second waited, so it did not rewrite the
block under the first.

Lateness is asserted, never assumed: an event recorded on A right behind the late edit (or call) must still be incomplete
immediately after the call under test has been enqueued; for a call that returns only when its work is done (host form, or
synchronous) immediately before it.  No case that runs is excused.

The ballast is volume_support.BALLAST_FILLS = 2048 whole-volume fills of a 512^3 volume (two per module, so that the cases
with two late streams touch no volume from two streams), the items of one
device-memory vrc_volume_fill_boxes list, so that the backlog stands when that one call returns.  Measured on the MI355X:
27.5 ms per ballast; the longest host-side enqueue of a call that stays asynchronous 0.81 ms (vrc_levels_reduce in device
form), 34 times shorter; the margin asked for is 4 (test_the_ballast_outlasts_the_longest_enqueue_four_times holds it
whenever the cases of this file ran before it in the same process, and prints both figures; run alone it only measures).  A call that returns only when done takes up to 53 ms here, ballast included; its edit
is held to be incomplete BEFORE the call.

Besides the result every case checks that vrc_last_error() is what it was before the case -- not that it is empty, which was
the plan: the text is never cleared, so an earlier file's refusal may still stand there; every return code is checked --, that vrc_volume_edit_scratch_bytes changes
only for the volumes whose record says it may, and that after a torch.cuda.synchronize() a plain download still equals the
model: a late writer would show there.

Not asserted, on purpose: the table says a device-memory LIST edit (set_voxels, fill_boxes, fill_spheres, fill_capsules,
raster_mesh) is not ordered against edits on other streams.  Those rows have a waits-for case in host form only; whatever a
device-form list edit does against a late edit on another stream is an accident, and no case here encodes it.

Such a test can show a missing wait or record; it cannot prove a present one."""
import time

import numpy as np
import pytest

import ordering_cases as oc
from volume_support import Ballast, Stream, event_on, device_words, volume_of

pytestmark = pytest.mark.gpu

ENQUEUE_MS = {}                          # case id -> host time of the call under test, for the margin test at the end


@pytest.fixture(scope="module")
def ballasts(built):
    """two 512^3 ballast volumes: the cases with two late roles keep two streams busy, each with a volume of its own"""
    pair = [Ballast(), Ballast()]
    yield pair
    for b in pair:
        b.close()


@pytest.fixture(scope="module")
def ballast(ballasts):
    return ballasts[0]


def case_list():
    out = []
    for r in oc.RECORDS:
        roles = list(r.waits)
        groups = [(role,) for role in roles] + ([tuple(roles)] if len(roles) > 1 and r.stream == "NULL" else [])
        for late in groups:
            for form in r.forms:
                if all(form in r.waits[role] for role in late):
                    out.append(pytest.param(r.name, "waits", late, form, id=f"{r.name}-waits-{'+'.join(late)}-{form}"))
        if r.recorded and not r.returns_when_done(oc.DEVICE):     # vrc_volume_flood: see the docstring
            out.append(pytest.param(r.name, "recorded", (), oc.DEVICE, id=f"{r.name}-recorded"))
    return out


class Subjects:
    def __init__(self, record):
        import cpuvoxelraycaster_amd as vrc
        self.L = vrc.capi.load()
        self.vol = {role: volume_of(content) for role, content in record.subjects.items()}
        self.scratch = {role: v.editScratchBytes() for role, v in self.vol.items()}
        self.error = self.L.vrc_last_error()
        self.record = record

    def check(self, want_out, want_vols, out):
        import torch
        assert oc.canon(out) == oc.canon(want_out)
        for role, v in self.vol.items():
            assert np.array_equal(v.download(), want_vols[role]), role
        assert self.L.vrc_last_error() == self.error
        for role, v in self.vol.items():
            if role not in self.record.scratch:
                assert v.editScratchBytes() == self.scratch[role], role
            else:
                assert v.editScratchBytes() >= self.scratch[role], role
        torch.cuda.synchronize()
        for role, v in self.vol.items():
            assert np.array_equal(v.download(), want_vols[role]), role       # nothing was written late

    def close(self):
        for v in self.vol.values():
            v.close()


def timed(case, generator):
    t = time.perf_counter()
    next(generator)
    ENQUEUE_MS[case] = (time.perf_counter() - t) * 1e3


def run_waits(record, late, form, ballasts, case):
    import torch
    s, e, entered = Subjects(record), None, []
    try:
        edits = {role: device_words(oc.edit_voxels(record.subjects[role].shape[0])) for role in late}
        for _ in range(len(late) + (record.stream != "NULL")):
            entered.append(Stream())
            entered[-1].__enter__()
        handles = [st.h for st in entered]
        e = oc.Env(s.vol, form, handles[-1] if record.stream != "NULL" else None)
        g = record.run(e)
        next(g)                                                   # lists uploaded, snapshots taken
        torch.cuda.synchronize()
        events = []
        for role, a, ballast in zip(late, handles, ballasts):     # a ballast volume per late stream: no volume on two streams
            ballast.enqueue(a)
            s.vol[role].setVoxelsDevice(edits[role].numel() // 3, edits[role].data_ptr(), True, a)
            events.append(event_on(a))
        if record.returns_when_done(form):
            assert not any(ev.query() for ev in events), "the edit was not late: it had landed before the call"
            timed(case, g)
        else:
            timed(case, g)
            assert not any(ev.query() for ev in events), "the edit was not late: it had landed before the call was enqueued"
        torch.cuda.synchronize()
        out = next(g)
        want_out, want_vols = record.outcome(late)
        s.check(want_out, want_vols, out)
    finally:
        torch.cuda.synchronize()                                  # a failed case leaves nothing in flight for the next one
        for st in entered:
            st.__exit__(None, None, None)
        if e is not None:
            e.close()
        s.close()


def run_recorded(record, ballast, case):
    import torch
    s, envs = Subjects(record), []
    want_out, want_vols = record.outcome(())
    role = record.recorded
    try:
        with Stream() as a, Stream() as b:
            if record.extractor:
                first, second = oc.Env(s.vol, oc.DEVICE, a, oc.WINDOW), oc.Env(s.vol, oc.DEVICE, b, oc.SECOND_WINDOW)
                envs += [first, second]
                g1, g2 = record.run(first), record.run(second)
                next(g1), next(g2)
                torch.cuda.synchronize()
                ballast.enqueue(a)
                timed(case, g1)
                late = event_on(a)
                next(g2)
                assert not late.query(), "the first extraction was not late: it had finished before the second was enqueued"
                # both lists come out right in either order; what the record does is make B wait: once B is done, A is
                s.L.vrc_stream_synchronize(0, b)
                assert late.query(), "the second extraction did not wait for the first"
                torch.cuda.synchronize()
                assert oc.canon(next(g1)) == oc.canon(record.model(dict(record.subjects), oc.WINDOW)[0])
                assert oc.canon(next(g2)) == oc.canon(record.model(dict(record.subjects), oc.SECOND_WINDOW)[0])
                s.check(None, want_vols, None)
            else:
                e = oc.Env(s.vol, oc.DEVICE, a)
                envs.append(e)
                g = record.run(e)
                next(g)
                torch.cuda.synchronize()
                ballast.enqueue(a)
                timed(case, g)
                late = event_on(a)
                assert not late.query(), "the call was not late: it had finished before the download"
                got = s.vol[role].download()                      # the NULL stream, no synchronisation in between
                assert np.array_equal(got, want_vols[role])
                torch.cuda.synchronize()
                s.check(want_out, want_vols, next(g))
    finally:
        torch.cuda.synchronize()
        for e in envs:
            e.close()
        s.close()


@pytest.mark.parametrize("name, direction, late, form", case_list())
def test_ordering(built, ballasts, ballast, request, name, direction, late, form):
    record = oc.by_name()[name]
    if direction == "waits":
        run_waits(record, late, form, ballasts, request.node.callspec.id)
    else:
        run_recorded(record, ballast, request.node.callspec.id)


def test_commit_behind_a_late_edit_is_the_scene_of_the_edited_volume(built, ballast):
    """the committed scene against LSVO.fromVolume of the post-edit model, as well as against the oracle's compiler"""
    import torch
    import cpuvoxelraycaster_amd as vrc
    record = oc.by_name()["vrc_volume_commit"]
    vol = record.subjects["v"]
    volume, edit = volume_of(vol), device_words(oc.edit_voxels(vol.shape[0]))
    torch.cuda.synchronize()
    with Stream() as a:
        ballast.enqueue(a)
        volume.setVoxelsDevice(edit.numel() // 3, edit.data_ptr(), True, a)
        late = event_on(a)
        assert not late.query(), "the edit was not late"
        svo = volume.commit()
    want = vrc.LSVO.fromVolume(oc.edited(vol), oc.DEPTH)
    assert svo.downloadNodes().tobytes() == want.downloadNodes().tobytes()
    for h in (svo, want, volume):
        h.close()


def test_the_ballast_outlasts_the_longest_enqueue_four_times(built, ballast):
    """the ballast's duration by events against the longest host-side enqueue of the cases that ran before this test"""
    import torch
    with Stream() as a:
        ext = torch.cuda.ExternalStream(a.value)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record(ext)
        ballast.enqueue(a)
        end.record(ext)
        end.synchronize()
        ballast_ms = start.elapsed_time(end)
    assert ballast_ms > 0
    if not ENQUEUE_MS:                       # run alone: no case of this file ran before, nothing to compare the ballast with
        return
    asynchronous = {c: ms for c, ms in ENQUEUE_MS.items()
                    if not oc.by_name()[c.split("-")[0]].returns_when_done(oc.HOST if c.endswith("-host") else oc.DEVICE)}
    case, longest = max(asynchronous.items(), key=lambda kv: kv[1])
    print(f"ballast {ballast_ms:.3f} ms for {ballast.fills} fills; longest asynchronous enqueue {longest:.3f} ms ({case}); "
          f"{len(ENQUEUE_MS)} cases; longest call that returns when done {max(ENQUEUE_MS.values()):.3f} ms")
    assert ballast_ms >= 4 * longest, (ballast_ms, case, longest)
