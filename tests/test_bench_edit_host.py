"""tools/bench_edit.py without a GPU: the mode table against the committed profiles, which mode and which depths a command
line selects, what run() prints and writes, and the values of its pure helpers."""
import glob
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("bench_edit_tool", os.path.join(ROOT, "tools", "bench_edit.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.fixture(scope="module")
def tool():
    return load_tool()


def selected(tool, *argv):
    return tool.select(tool.make_parser().parse_args(list(argv)))


def test_importing_the_tool_imports_neither_torch_nor_the_package():
    """in a fresh interpreter: in this one another test may have imported them already"""
    code = ("import sys, importlib.util\n"
            "spec = importlib.util.spec_from_file_location('bench_edit_tool', sys.argv[1])\n"
            "tool = importlib.util.module_from_spec(spec)\n"
            "spec.loader.exec_module(tool)\n"
            "bad = [m for m in sys.modules if m.split('.')[0] in ('torch', 'cpuvoxelraycaster_amd', '__graft_entry__')]\n"
            "assert not bad, bad\n")
    subprocess.check_call([sys.executable, "-c", code, os.path.join(ROOT, "tools", "bench_edit.py")])


def test_mode_table_matches_the_parser_and_the_committed_profiles(tool):
    names, flags = [m.name for m in tool.MODES], [m.flag for m in tool.MODES if m.flag]
    assert len(set(names)) == len(names) == 20 and len(set(flags)) == len(flags) == 19
    assert [m.flag for m in tool.MODES].count(None) == 1 and tool.MODES[-1].flag is None and tool.MODES[-1].bench is tool.bench_depth
    assert names == ["columns", "pack", "cells", "delta", "fracture", "clearance", "pair_contacts", "contacts", "rigid", "fall", "travel",
                     "rects", "stamp", "distance", "components", "surface", "voxelize", "flood", "brushes", "edit"]
    assert [m.name for m in tool.MODES if m.writes] == names[:15]
    options = sorted(s for a in tool.make_parser()._actions for s in a.option_strings if s not in ("-h", "--help"))
    assert options == sorted(flags + ["--depths", "--pairs"])
    by_name = {m.name: m for m in tool.MODES}
    seen = 0
    for path in glob.glob(os.path.join(ROOT, "profiles", "edit", "bench_*.json")):
        doc = json.load(open(path))
        if isinstance(doc, dict) and "bench" in doc:
            mode = by_name[os.path.basename(path)[len("bench_"):-len(".json")]]
            assert doc["bench"] == mode.label and os.path.basename(path) == mode.file, path
            seen += 1
    assert seen >= 15
    assert tool.make_parser().description == tool.__doc__


def test_the_first_mode_in_table_order_is_selected(tool):
    assert selected(tool)[0] is tool.MODES[-1] and selected(tool)[0].label == "edit"
    assert selected(tool, "--contacts", "--distance")[0].name == "contacts"
    assert selected(tool, "--distance", "--contacts")[0].name == "contacts"
    assert selected(tool, "--columns", "--brushes")[0].name == "columns"
    for mode in tool.MODES[:-1]:
        assert selected(tool, mode.flag)[0] is mode and mode.label == "edit_" + mode.name


def test_depths_default_per_mode_and_are_kept_when_given(tool):
    for mode in tool.MODES:
        flag = [mode.flag] if mode.flag else []
        want = [8, 9, 10] if mode.flag is None else [9, 10] if mode.name == "brushes" else [9]
        assert selected(tool, *flag) == (mode, want)
        assert selected(tool, *flag, "--depths", "7") == (mode, [7])
    assert selected(tool, "--depths", "8", "9", "10", "--columns")[1] == [8, 9, 10]
    assert selected(tool, "--brushes", "--depths", "8", "9", "10")[1] == [8, 9, 10]


def test_run_prints_one_line_and_writes_only_a_writing_modes_file(tool, tmp_path, capsys):
    calls = []
    package = object()

    def bench(vrc, depth, pairs):
        calls.append((vrc, depth, pairs))
        return {"size": 1 << depth, "ms": {"median": 0.5}}

    writing = tool.MODES[0]._replace(bench=bench)
    assert writing.writes
    out = tool.run(writing, [10, 7], 0, package, "a device", str(tmp_path))
    want = {"bench": "edit_columns", "device": "a device",
            "depths": {"10": {"size": 1024, "ms": {"median": 0.5}}, "7": {"size": 128, "ms": {"median": 0.5}}}}
    assert out == want and list(out) == ["bench", "device", "depths"] and list(out["depths"]) == ["10", "7"]
    assert calls == [(package, 10, 1), (package, 7, 1)]                       # pairs = 0 runs as one pair
    assert capsys.readouterr().out == json.dumps(want) + "\n"
    assert os.listdir(tmp_path) == ["bench_columns.json"]
    assert open(tmp_path / "bench_columns.json", "rb").read() == (json.dumps(want, indent=1) + "\n").encode()

    silent = tool.MODES[-1]._replace(bench=bench)
    assert not silent.writes
    empty = tmp_path / "empty"
    empty.mkdir()
    del calls[:]
    out = tool.run(silent, [8], 3, package, "a device", str(empty))
    assert out["bench"] == "edit" and calls == [(package, 8, 3)]
    assert capsys.readouterr().out == json.dumps(out) + "\n"
    assert os.listdir(empty) == []


def test_pure_helpers_keep_their_values(tool):
    assert tool.stat([3, 1, 2], 4) == {"median": 2, "min": 1, "max": 3}
    assert list(tool.stat([3, 1, 2], 4)) == ["median", "min", "max"]
    assert tool.stat([0.123456789, 0.2, 0.3000049]) == {"median": 0.2, "min": 0.12346, "max": 0.3}
    assert tool.stat([1.23456, 2.34567], 3) == {"median": 1.79, "min": 1.235, "max": 2.346}
    # (piece, destination word) items, a word = 2 x 2 x 8 voxels; along z the count is vrc_box_words.h's bound for any alignment
    assert tool.box_words([[4, 4, 4, 4, 9, 9]]) == 0                           # empty along x
    assert tool.box_words([[5, 5, 5, 6, 6, 6]]) == 1                           # one voxel
    assert tool.box_words([[0, 0, 6, 2, 2, 10]]) == 2                          # z = 6 .. 9 lies in two words
    assert tool.box_words([[0, 0, 0, 2, 2, 8]]) == 2
    assert tool.box_words([[3, 7, 62, 10, 9, 67]]) == 16
    assert tool.box_words([[0, 0, 0, 512, 512, 512]]) == 4259840
    assert tool.box_words([[4, 4, 4, 4, 9, 9], [5, 5, 5, 6, 6, 6], [0, 0, 6, 2, 2, 10], [0, 0, 0, 512, 512, 512]]) == 4259843
    cuts, slab = tool.fall_cuts(512)
    assert cuts[0] == [0, 281, 0, 512, 285, 512] and cuts[1] == [0, 301, 0, 512, 304, 512] and slab == [[0, 257, 0, 512, 258, 512]]
    assert len(cuts) == 2 + 2 * 16 and cuts[2] == [30, 281, 0, 32, 512, 512] and cuts[-1] == [0, 281, 510, 512, 512, 512]
