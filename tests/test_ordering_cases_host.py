"""tests/ordering_cases.py against the table "Ordering of the volume's entry points" of DESIGN.md and the prototypes of
include/vrc.h, on the CPU: every vrc_* function that takes a vrc_volume* has a row; every row that waits for a volume or is
recorded as an edit of one has a record whose stream, roles, forms and synchrony are the row's; and every record's case can
tell a call that waited from one that did not -- what a test observes with the call behind the late edit differs, by the
numpy models alone, from what it observes had the call run before the edit landed."""
import os
import re

import pytest

import ordering_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLES = ("v", "src", "dst", "region", "medium", "seeds", "world", "fixed", "before", "after")


def table_rows(text):
    """{entry point: (stream, waits-for cell, recorded cell, synchronous cell)} of the table's rows"""
    at = text.index("**Ordering of the volume's entry points.**")
    lines = text[at:].split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("| entry point |"))
    rows = {}
    for line in lines[start + 2:]:
        if not line.startswith("|"):
            break
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        assert len(cells) == 5, line
        names, last = [], None
        for token in re.findall(r"`([^`]+)`", cells[0]):
            if token.startswith("vrc_"):
                last = token
            else:
                assert token.startswith("_") and last, line          # `vrc_labels_count` / `_depth`: the same family
                token = "_".join(last.split("_")[:2]) + token
            names.append(token)
        assert names, line
        for name in names:
            assert name not in rows, name
            rows[name] = tuple(cells[1:])
    return rows


def roles_of(cell):
    """the roles a cell names before its first parenthesis: 'src and dst', 'v, in host form only (...)', 'fixed, where given'"""
    head = cell.split("(")[0].split(";")[0]
    if head.startswith("--") or head.startswith("the whole device"):
        return []
    roles = []
    for word in re.findall(r"[a-z]+", head.split(",")[0]):           # 'src and dst', 'v in device form': the leading role names
        if word in ROLES:
            roles.append(word)
        elif word != "and":
            break
    assert roles, cell
    return roles


def row_of(cells):
    """(stream, {role: forms}, recorded role, synchrony) as a Record states them"""
    stream, waits, recorded, sync = cells
    stream = "NULL" if stream.startswith("NULL") else "caller's" if stream.startswith("caller's") else stream
    forms = (oc.HOST,) if "in host form only" in waits.split("(")[0] else oc.BOTH
    recorded_roles = roles_of(recorded)
    assert len(recorded_roles) <= 1, recorded
    sync = "yes" if sync.startswith("yes") else "no" if sync.startswith("no") else "host / device" if sync.startswith("host / device") else sync
    return stream, {role: forms for role in roles_of(waits)}, (recorded_roles[0] if recorded_roles else None), sync


def prototypes(text):
    """{function: argument text} of every vrc_* prototype, comments taken out"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(vrc_\w+)\s*\(([^;{}()]*)\)\s*;", text)}


@pytest.fixture(scope="module")
def rows():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        return table_rows(f.read())


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "vrc.h")) as f:
        return f.read()


def missing_rows(header_text, rows):
    return sorted(name for name, args in prototypes(header_text).items() if re.search(r"\bvrc_volume\s*\*", args) and name not in rows)


def test_every_entry_point_that_takes_a_volume_has_a_row(rows, header):
    protos = prototypes(header)
    assert len(protos) > 150 and "vrc_morph_apply" in protos and "vrc_volume_flood" in protos      # the multi-line ones too
    assert missing_rows(header, rows) == []
    assert sorted(name for name in rows if name not in protos) == []                               # and no row of a call that is gone
    # the check can fail: a prototype added without a row is named
    assert missing_rows(header + "\nint vrc_volume_frobnicate(vrc_volume *v,\n        void *stream);\n", rows) == ["vrc_volume_frobnicate"]


def test_every_row_that_orders_has_a_record(rows):
    records = oc.by_name()
    assert len(records) == len(oc.RECORDS)                                                         # no name twice
    ordering = sorted(name for name, cells in rows.items() if row_of(cells)[1] or row_of(cells)[2])
    assert len(ordering) >= 46
    assert sorted(records) == ordering


@pytest.mark.parametrize("name", sorted(oc.by_name()))
def test_the_record_states_the_row(rows, name):
    record = oc.by_name()[name]
    stream, waits, recorded, sync = row_of(rows[name])
    assert record.stream == stream
    # a call without a memory kind has one form (record.forms) and waits in it; its record still says the row's words
    assert {role: tuple(forms) for role, forms in record.waits.items()} == waits
    assert set(record.waits) == set(waits)
    assert record.recorded == recorded
    assert record.sync == sync
    assert set(record.subjects) >= set(waits) | ({recorded} if recorded else set())
    assert set(record.scratch) <= set(record.subjects)
    assert record.forms in (oc.BOTH, (oc.DEVICE,))
    for role, vol in record.subjects.items():
        assert vol.shape[0] in (4, 16, 32) and vol.shape == (vol.shape[0],) * 3, role


@pytest.mark.parametrize("name", sorted(oc.by_name()))
def test_the_case_tells_a_call_that_waited_from_one_that_did_not(name):
    record = oc.by_name()[name]
    quiet = record.outcome(())
    groups = [(role,) for role in record.waits] + ([tuple(record.waits)] if len(record.waits) > 1 else [])
    for late in groups:
        waited, early = record.outcome(late), record.mistimed(late)
        assert oc.canon(waited) != oc.canon(early), late
        if oc.canon(waited) == oc.canon(quiet):                   # the edit itself shows, unless the call writes that volume whole
            assert set(late) <= set(record.model(dict(record.subjects))[1]), late
    if record.recorded and not record.extractor:
        # the recorded-as direction reads the volume behind the call: the call must change it
        assert oc.canon(quiet[1][record.recorded]) != oc.canon(record.subjects[record.recorded])
    if record.extractor:
        a, b = record.model(dict(record.subjects), oc.WINDOW)[0], record.model(dict(record.subjects), oc.SECOND_WINDOW)[0]
        assert oc.canon(a) != oc.canon(b) and len(a[1]) == oc.WINDOW[1] and len(b[1]) == oc.SECOND_WINDOW[1]
    for vol in record.subjects.values():
        assert not vol.flags.writeable                             # the subjects are shared between cases


def test_the_late_edit_changes_every_subject():
    for record in oc.RECORDS:
        for role, vol in record.subjects.items():
            assert oc.canon(oc.edited(vol)) != oc.canon(vol), (record.name, role)


def test_removing_a_record_is_noticed(rows, monkeypatch):
    monkeypatch.setattr(oc, "RECORDS", [r for r in oc.RECORDS if r.name != "vrc_travel_field"])
    with pytest.raises(AssertionError):
        test_every_row_that_orders_has_a_record(rows)
