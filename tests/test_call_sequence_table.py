"""What tests/test_gpu_call_sequences.py rests on, checked without a GPU: the step table of tests/call_sequences.py names every `_dev` entry
point of the binding and every call that sets or reserves something on a context, and the shapes of the "new layouts behind dirt" test
are small enough for the dirt to lie where the successors carve (the layout headers compiled with g++, tests/c/seq_layout_dump.cpp)."""
import os
import subprocess

import call_sequences as cs
from conftest import ROOT
from fourq_amd import _lib


def test_the_step_table_names_every_dev_entry_point():
    cs.check_entry_points()


def test_every_call_that_sets_or_reserves_has_a_state_kind_or_a_reason():
    cs.check_state_calls()
    assert "fourq_ctx_set_host_timing" in cs.EXEMPT_STATE_CALLS and all(len(reason) > 20 for reason in cs.EXEMPT_STATE_CALLS.values())


def test_a_later_family_without_a_kind_fails_both_checks(monkeypatch):
    """the two checks bite: a `_dev` call or a setter that the table does not name makes them fail"""
    import pytest
    monkeypatch.setitem(_lib.PROTOTYPES, "fourq_x_foo_dev", _lib.PROTOTYPES["fourq_vrf_reserve"])
    with pytest.raises(AssertionError, match="fourq_x_foo_dev"):
        cs.check_entry_points()
    monkeypatch.delitem(_lib.PROTOTYPES, "fourq_x_foo_dev")
    cs.check_entry_points()
    monkeypatch.setitem(_lib.PROTOTYPES, "fourq_x_set", _lib.PROTOTYPES["fourq_vrf_reserve"])
    with pytest.raises(AssertionError, match="fourq_x_set"):
        cs.check_state_calls()


def test_the_dirty_region_covers_every_successors_layout(tmp_path):
    """mul_bytes at 4 099 rows rewrites rows_in and rows_out, bytes [0, 320 x 4099) of the work buffer (MulRows: 20 + 20 words per row in
    front of everything else); every successor of the dirt test carves its whole layout inside them.  The figures are those measured
    when the shapes were chosen."""
    exe = str(tmp_path / "seq_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"), os.path.join(ROOT, "tests", "c", "seq_layout_dump.cpp"), "-o", exe],
                   check=True)
    args = [str(a) for _, _, layout in cs.DIRT_SUCCESSORS for a in layout]
    out = subprocess.run([exe] + args + ["MulRows", str(cs.DIRT_ROWS)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = [line.split() for line in out if line]
    assert len(got) == len(cs.DIRT_SUCCESSORS) + 1
    dirty = 320 * cs.DIRT_ROWS
    assert dirty == 1311680 and int(got[-1][4]) >= dirty                      # the predecessor's own layout reaches past its two row regions
    sizes = {}
    for (name, kw, layout), line in zip(cs.DIRT_SUCCESSORS, got):
        assert line[0] == layout[0] and 0 < int(line[4]) <= dirty, (name, kw, line)
        sizes[" ".join(str(a) for a in layout)] = int(line[4])
    measured = {"Keyset 257": 166528, "Commit 257 1": 25696, "Bucket 1 257 4": 421520, "Bucket 3 65 4": 776176, "Dleq 255 5": 112256, "Vrf 257": 312448, "Shamir 51 5": 124640}
    assert {k: sizes[k] for k in measured} == measured
    assert {line[0] for line in got} == {"Keyset", "Commit", "Bucket", "MsmRagged", "Dleq", "Vrf", "Shamir", "MulRows"}       # the seven later layouts, each at least once
