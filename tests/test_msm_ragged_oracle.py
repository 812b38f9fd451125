"""Pins the host side of the ragged grouped sums (fourq_raggedsum_*, fourq_amd/csrc/msm_shape.h) before any GPU runs (no GPU needed).

The planner turns validated row offsets into the geometry of every fold pass.  tests/c/msm_shape_dump.cpp, a stand-alone program with its own
main, prints what it plans, and this file restates the rules in Python: levels L_p[g] = max(1, ceil(L_{p-1}[g] / 64)), passes until every
group has one row, one descriptor {first, count <= 64} per output row that together partition the level below exactly and in order, a
uniform team width min(16, 2^ceil(log2(largest count))), and a work-buffer layout whose regions hold every level.  The same program runs
once more built with the address and undefined-behaviour sanitizers -- as a plain executable, never loaded into Python.  The rest: the
seven symbols in header and binding, and the ABI version."""
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

FOLD, TEAM_MAX, CAP = 64, 16, 0xffffff00
A = [0, 1, 0, 0, 2, 63, 64, 65, 0, 127, 129, 1, 0]
B = [4097, 0, 1]
C = [1] * 67
D = [0] * 5
E = [3, 5, 31, 33, 17]
EQ = [65] * 3
FIXED = {"A": A, "B": B, "C": C, "D": D, "E": E, "Eq": EQ, "one": [1], "empty": [0], "F^3+1": [64 ** 3 + 1, 0]}
SYMBOLS = {"fourq_raggedsum_shape_set": 3, "fourq_raggedsum_shape_count": 3, "fourq_raggedsum_shape_reserve": 1, "fourq_raggedsum_affine": 4,
           "fourq_raggedsum_affine_dev": 4, "fourq_raggedsum_bytes": 5, "fourq_raggedsum_bytes_dev": 5}
SOURCES = ["-I", os.path.join(ROOT, "fourq_amd", "csrc"), os.path.join(ROOT, "tests", "c", "msm_shape_dump.cpp")]


def offsets_of(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


def random_shapes():
    """200 seeded shapes: n <= 20 000, groups <= 300, empty groups allowed; short groups, groups around the fold factor and a few long ones"""
    rng = random.Random(8100)
    shapes = []
    while len(shapes) < 200:
        groups = rng.randint(1, 300)
        kind = rng.randrange(4)
        pick = [lambda: rng.randint(0, 3), lambda: rng.choice([0, 1, 63, 64, 65, 127, 128, 129]), lambda: rng.randint(0, 200),
                lambda: rng.choice([0, 0, 1, 2, rng.randint(0, 9000)])][kind]
        lengths = [pick() for _ in range(groups)]
        if sum(lengths) <= 20000:
            shapes.append(lengths)
    return shapes


def a256(n):
    return (n + 255) // 256 * 256


def parse(text):
    """the dump's lines -> one dict per shape (None for a refused one)"""
    shapes = []
    for line in text.splitlines():
        words = line.split()
        if words[0] == "shape":
            if words[2] == "invalid":
                shapes.append(None)
            else:
                shapes.append({"groups": int(words[3]), "rows": int(words[5]), "n_passes": int(words[7]), "passes": []})
        elif words[0] == "pass":
            shapes[-1]["passes"].append({k: int(v) for k, v in zip(words[2::2], words[3::2])})
        elif words[0] == "desc":
            shapes[-1]["passes"][-1]["desc"] = [tuple(int(x) for x in w.split(":")) for w in words[1:]]
        elif words[0] == "layout":
            shapes[-1]["layout"] = {k: int(v) for k, v in zip(words[1::2], words[2::2])}
        else:
            raise AssertionError(line)
    return shapes


def run(exe, offset_lists, cap=CAP):
    """The plans of many shapes; at most 40 per process, so that no command line grows past what the system takes"""
    plans = []
    for at in range(0, len(offset_lists), 40):
        args = []
        for offs in offset_lists[at:at + 40]:
            args += ([] if not args else ["/"]) + [str(o) for o in offs]
        proc = subprocess.run([exe, str(cap)] + args, capture_output=True, text=True)
        assert proc.returncode == 0, (proc.returncode, proc.stderr[-2000:])
        assert not proc.stderr, proc.stderr[-2000:]
        plans += parse(proc.stdout)
    assert len(plans) == len(offset_lists)
    return plans


def check_plan(lengths, plan):
    """Every rule of the header's comment, from the lengths alone"""
    groups, n = len(lengths), sum(lengths)
    assert plan is not None and (plan["groups"], plan["rows"]) == (groups, n)
    level = list(lengths)
    want_passes = 0
    assert plan["n_passes"] == len(plan["passes"])
    for p in plan["passes"]:
        assert any(m != 1 for m in level)                                   # a pass runs only while some group is not at one row
        nxt = [max(1, -(-m // FOLD)) for m in level]
        assert p["rows_in"] == sum(level) and p["rows_out"] == sum(nxt) == len(p["desc"])
        # the partition: descriptor after descriptor covers the level below exactly once and in order, group after group
        at, t = 0, 0
        for m, out in zip(level, nxt):
            covered = 0
            for _ in range(out):
                first, count = p["desc"][t]
                assert first == at and 0 <= count <= FOLD and count == min(FOLD, m - covered), (t, first, count)
                at, covered, t = at + count, covered + count, t + 1
            assert covered == m
        assert at == sum(level) and t == len(p["desc"])
        largest = max(c for _, c in p["desc"])
        team = 1
        while team < TEAM_MAX and team < largest:
            team *= 2
        assert (p["largest"], p["team"], p["iters"]) == (largest, team, max(1, -(-largest // team)))
        assert p["team"] * p["iters"] >= largest and p["team"] * p["iters"] <= FOLD
        level = nxt
        want_passes += 1
    assert all(m == 1 for m in level)                                       # ... and the passes end with one row per group
    longest = max(lengths)
    by_formula = 0 if all(m == 1 for m in lengths) else max(1, next(k for k in range(8) if FOLD ** k >= longest))
    assert want_passes == by_formula, (want_passes, by_formula)
    # the layout: regions in order, 16-byte aligned, disjoint, inside bytes(); the two fold regions hold the levels written to them
    lay = dict(plan["layout"])
    total = lay.pop("bytes")
    ladder = max(n, 1)
    level1, level2 = groups + n // FOLD, groups + (groups + n // FOLD) // FOLD
    need = {"rows_in": ladder * 160, "rows_out": ladder * 160, "st_decode": ladder, "part_a": level1 * 96, "st_a": level1, "part_b": level2 * 96, "st_b": level2}
    assert list(lay) == list(need)
    spans = [(lay[k], lay[k] + need[k], k) for k in need]
    assert spans[0][0] == 0 and spans == sorted(spans)
    for (_, end, name), (start, _, nxt_name) in zip(spans, spans[1:]):
        assert end <= start, (name, nxt_name)
    assert all(s % 16 == 0 and e <= total for s, e, _ in spans)
    assert total == 2 * ladder * 160 + a256(ladder) + level1 * 96 + a256(level1) + level2 * 96 + a256(level2)
    for i, p in enumerate(plan["passes"]):
        assert p["rows_out"] <= (level1 if i % 2 == 0 else level2), (i, p["rows_out"])


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / "msm_shape_dump")
    proc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + SOURCES + ["-o", exe], capture_output=True, text=True)
    return exe, proc


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe, proc = build(tmp_path_factory, "msm_shape", ["-O1"])
    assert proc.returncode == 0, proc.stderr[-3000:]
    return exe


# ---- 1. the planner against its restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_shapes_are_planned_by_the_rules(dump, name):
    lengths = FIXED[name]
    plan, = run(dump, [offsets_of(lengths)])
    check_plan(lengths, plan)
    passes = {"A": 2, "B": 3, "C": 0, "D": 1, "E": 1, "Eq": 2, "one": 0, "empty": 1, "F^3+1": 4}[name]
    assert plan["n_passes"] == passes
    if name == "E":
        assert plan["passes"][0]["team"] == 16 and plan["passes"][0]["iters"] == 3       # 33 rows: 3 per lane, lanes idle in every other team
    if name == "D":
        assert plan["passes"][0]["desc"] == [(0, 0)] * 5 and (plan["passes"][0]["team"], plan["passes"][0]["iters"]) == (1, 1)
    if name == "A":
        assert [p["team"] for p in plan["passes"]] == [16, 4] and plan["passes"][1]["largest"] == 3


def test_random_shapes_are_planned_by_the_rules(dump):
    shapes = random_shapes()
    assert len(shapes) == 200 and max(len(s) for s in shapes) <= 300 and max(sum(s) for s in shapes) <= 20000
    assert any(0 in s for s in shapes) and any(max(s) > FOLD * FOLD for s in shapes) and any(max(s) <= 1 for s in shapes)
    for lengths, plan in zip(shapes, run(dump, [offsets_of(s) for s in shapes])):
        check_plan(lengths, plan)


def test_invalid_offsets_are_refused(dump):
    bad = {"a descending pair": [0, 5, 4, 9], "descending at the end": [0, 1, 0], "offsets[0] != 0": [1, 2, 3], "no group": [0], "nothing": []}
    for why, offs in bad.items():
        assert run(dump, [offs]) == [None], why
    # totals above the cap: the rows, and the groups
    assert run(dump, [[0, CAP + 1]]) == [None] and run(dump, [[0, 0xffffffff]]) == [None]
    assert run(dump, [[0, 50, 101]], cap=100) == [None] and run(dump, [[0] * 102], cap=100) == [None]
    ok, = run(dump, [[0, 50, 100]], cap=100)
    check_plan([50, 50], ok)
    ok, = run(dump, [[0] * 101], cap=100)
    check_plan([0] * 100, ok)
    # a refused shape between two good ones changes neither
    plans = run(dump, [offsets_of(A), [0, 3, 2], offsets_of(E)])
    assert plans[1] is None
    check_plan(A, plans[0])
    check_plan(E, plans[2])


# ---- 2. the same program under the sanitizers: a plain executable, nothing preloaded ------------------------------------------------------
def test_planner_runs_clean_under_address_and_undefined_sanitizers(tmp_path_factory):
    exe, proc = build(tmp_path_factory, "msm_shape_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if proc.returncode != 0 and re.search(r"asan|ubsan|sanitize", proc.stderr, re.I):
        pytest.skip("this compiler has no sanitizer runtime: " + proc.stderr.strip().splitlines()[-1][:200])
    assert proc.returncode == 0, proc.stderr[-3000:]
    shapes = list(FIXED.values()) + random_shapes()
    for lengths, plan in zip(shapes, run(exe, [offsets_of(s) for s in shapes])):
        check_plan(lengths, plan)
    assert run(exe, [[0, 5, 4], [1, 2], [0, 0xffffffff], []]) == [None] * 4


# ---- 3. header and binding ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_same_new_symbols():
    from fourq_amd import _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_raggedsum_\w+)\s*\(([^;{]*)\)\s*;", header))
    assert set(decls) == set(SYMBOLS) == {n for n in _lib.PROTOTYPES if "ragged" in n}
    for name, args in decls.items():
        arity = len([a for a in args.split(",") if a.strip()])
        assert arity == len(_lib.PROTOTYPES[name][1]) == SYMBOLS[name], name
        assert re.match(r"\s*(const\s+)?fourq_ctx\s*\*\s*ctx\b", args), name
    assert "groups" not in decls["fourq_raggedsum_affine_dev"] and "group_size" not in "".join(decls.values())       # n and groups come from the shape
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600
    from fourq_amd import Engine
    for m in ("msm_shape", "msm_shape_count", "msm_shape_reserve", "msm_ragged", "msm_ragged_bytes", "msm_ragged_dev", "msm_ragged_bytes_dev"):
        assert callable(getattr(Engine, m)), m
    # the equal-length family is as it was
    assert {n for n in _lib.PROTOTYPES if "msm" in n} == {"fourq_msm_affine_batch", "fourq_msm_affine_batch_dev", "fourq_msm_bytes_batch", "fourq_msm_bytes_batch_dev"}


def test_offsets_are_checked_in_python_before_the_library_sees_them():
    from fourq_amd import Engine
    import numpy as np
    assert Engine._offsets([0, 3, 3, 7]).dtype == np.uint32 and list(Engine._offsets(np.array([0, 2], dtype=np.int64))) == [0, 2]
    for bad in ([0], [], [[0, 1]], [0, -1], [0, 1 << 32], [0.0, 1.0]):
        with pytest.raises(ValueError):
            Engine._offsets(bad)


# ---- 4. the reference's own answers on one ragged shape (tests/golden/msm_ragged.json) -------------------------------------------------------
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    import ref_loader
    from conftest import GOLDEN
    if not ref_loader.available():
        pytest.skip("the reference is not mounted here")
    spec = importlib.util.spec_from_file_location("make_msm_ragged", os.path.join(GOLDEN, "make_msm_ragged.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "msm_ragged.json")) as fh:
        assert mod.generate() == fh.read()


def test_group_law_through_the_c_oracle_gives_the_fixture(golden):
    """What tests/test_gpu_msm_ragged.py builds its expectations on: every P is [t]G, and the group's sum is [(sum k_i t_i) mod N]G -- the
    neutral (0, 1), encoded 01 00 .. 00, for the groups of no rows."""
    import curve4q_oracle as o
    import oracle_c as oc
    from conftest import GOLDEN
    from fourq_amd import codec
    fx = golden("msm_ragged.json")
    groups = fx["groups"]
    assert os.path.getsize(os.path.join(GOLDEN, "msm_ragged.json")) < 64 * 1024
    lengths = [g["length"] for g in groups]
    assert lengths == list(fx["lengths"]) == [0, 1, 3, 0, 0, 2, 5, 0, 66]
    assert all(len(g["k"]) == len(g["t"]) == len(g["P"]) == len(g["P_enc"]) == g["length"] for g in groups)
    assert {0, 1, o.N - 1, o.N, o.N + 1, (1 << 256) - 1} <= {g["k"][i] for g in groups if g["length"] >= 2 for i in (0, -1)}
    table = oc.table(oc.ENDO, codec.pack_point(o.AffineToR1(o.Gx, o.Gy)))
    ts = [t for g in groups for t in g["t"]]
    assert codec.unpack_points(oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(ts), None, table))) == [P for g in groups for P in g["P"]]
    sums = [sum(k * t for k, t in zip(g["k"], g["t"])) % o.N for g in groups]
    want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, table))
    assert codec.unpack_points(want) == [g["R"] for g in groups]
    assert [bytes(r).hex() for r in oc.encode(want)] == ["%064x" % g["R_enc"] for g in groups]
    for g in groups:
        if not g["length"]:
            assert g["R"] == ((0, 0), (1, 0)) and "%064x" % g["R_enc"] == "01" + "00" * 31
