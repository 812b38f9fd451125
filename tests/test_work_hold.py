"""The book of a buffer while calls are using it (fq_work::Hold in fourq_amd/csrc/work_layout.h, plain C++): compiled with g++ and driven on the
CPU the way WorkScope in fourq_amd.hip drives it (tests/c/work_hold_dump.cpp, a stand-alone program with its own main).  The outermost call
that opens a layout may grow the buffer; while its layout is open, a layout opened by a call it makes must end within the extent its parent
admits for inner calls and within what the buffer holds, or it is refused and nothing changes; closing puts the parent's book back.  The
staging buffer and the projective planes keep the same book with the whole buffer as the extent.  The same program runs once more built
with the address and undefined-behaviour sanitizers -- as a plain executable, never loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "work_hold_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "work_hold_dump.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def hold(request, tmp_path_factory):
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = build(tmp_path_factory, "work_hold_" + request.param, flags)

    def run(buffer, *ops):
        """ops: ("open", need, extent) or "close"  ->  one tuple per op: ("admit", depth, held, extent, grew) / ("refuse" | "close", depth, held, extent)"""
        argv = [op if op == "close" else "open:%d:%d" % op[1:] for op in ops]
        out = subprocess.run([exe, str(buffer), *argv], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
        assert len(out) == len(ops)
        return [(line.split()[0], *map(int, line.split()[1:])) for line in out]
    return run


def test_the_outermost_open_may_grow_and_the_next_one_after_it_closed_may_again(hold):
    assert hold(100, ("open", 100, 0), "close", ("open", 101, 0), "close", ("open", 1 << 40, 7), "close") == [
        ("admit", 1, 100, 0, 0), ("close", 0, 0, 0), ("admit", 1, 101, 0, 1), ("close", 0, 0, 0), ("admit", 1, 1 << 40, 7, 1), ("close", 0, 0, 0)]
    assert hold(0, ("open", 1, 1)) == [("admit", 1, 1, 1, 1)]


def test_a_nested_open_that_fits_is_admitted_at_depth_two_and_three(hold):
    # held stays what the outermost scope found; the extent is the innermost open layout's
    assert hold(1000, ("open", 1000, 600), ("open", 600, 200), ("open", 200, 0)) == [
        ("admit", 1, 1000, 600, 0), ("admit", 2, 1000, 200, 0), ("admit", 3, 1000, 0, 0)]
    assert hold(1000, ("open", 800, 600), ("open", 1, 1), ("open", 1, 0)) == [("admit", 1, 1000, 600, 0), ("admit", 2, 1000, 1, 0), ("admit", 3, 1000, 0, 0)]


def test_one_byte_over_the_extent_is_refused_and_changes_nothing(hold):
    assert hold(1000, ("open", 1000, 600), ("open", 601, 0), ("open", 600, 200), ("open", 201, 0), ("open", 200, 0)) == [
        ("admit", 1, 1000, 600, 0), ("refuse", 1, 1000, 600), ("admit", 2, 1000, 200, 0), ("refuse", 2, 1000, 200), ("admit", 3, 1000, 0, 0)]


def test_one_byte_over_the_held_bytes_is_refused_though_within_the_extent(hold):
    # a parent that declares more than the buffer holds (a wrong header): the nested call may still not make the buffer grow
    assert hold(1000, ("open", 1000, 5000), ("open", 1001, 0), ("open", 1000, 0)) == [("admit", 1, 1000, 5000, 0), ("refuse", 1, 1000, 5000), ("admit", 2, 1000, 0, 0)]


def test_a_leaf_parent_refuses_any_nested_layout(hold):
    assert hold(1000, ("open", 10, 0), ("open", 1, 0), ("open", 0, 0)) == [("admit", 1, 1000, 0, 0), ("refuse", 1, 1000, 0), ("admit", 2, 1000, 0, 0)]


def test_closing_restores_the_parents_extent_for_the_next_sibling(hold):
    got = hold(1000, ("open", 1000, 600), ("open", 600, 100), ("open", 101, 0), "close", ("open", 101, 0), ("open", 600, 0), ("open", 601, 0), "close", "close", ("open", 2000, 0))
    assert got == [("admit", 1, 1000, 600, 0), ("admit", 2, 1000, 100, 0), ("refuse", 2, 1000, 100), ("close", 1, 1000, 600), ("admit", 2, 1000, 0, 0), ("refuse", 2, 1000, 0),
                   ("refuse", 2, 1000, 0), ("close", 1, 1000, 600), ("close", 0, 0, 0), ("admit", 1, 2000, 0, 1)]


def test_a_buffer_held_whole_admits_what_it_holds_and_refuses_growth(hold):
    """The staging buffer under grouped_host and the planes under a scope that sized them: extent == held.  A user within it goes on, one
    that would have to grow it is refused, and once the holder is gone the buffer grows again."""
    assert hold(4096, ("open", 4096, 4096), ("open", 160, 4096), "close", ("open", 4096, 4096), "close", ("open", 4097, 4096), "close", ("open", 4097, 4097)) == [
        ("admit", 1, 4096, 4096, 0), ("admit", 2, 4096, 4096, 0), ("close", 1, 4096, 4096), ("admit", 2, 4096, 4096, 0), ("close", 1, 4096, 4096), ("refuse", 1, 4096, 4096),
        ("close", 0, 0, 0), ("admit", 1, 4097, 4097, 1)]
