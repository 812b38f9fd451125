"""The fixed-generator commitments before any GPU runs (no GPU needed): the restatement on the Python oracle (tests/commit_ref.py) against
the fixture made with the reference's point functions (tests/golden/commit.json) and against the group law; the symbols in header and
binding; and the launch geometry and work-buffer layout (fourq_amd/csrc/commit_layout.h) compiled with g++."""
import os
import re
import subprocess

import pytest

import commit_ref as ref
import curve4q_oracle as o
from conftest import ROOT, load_golden

SYMBOLS = ("fourq_commit_bases_set", "fourq_commit_bases_count", "fourq_commit_route", "fourq_commit_reserve", "fourq_commit_affine",
           "fourq_commit_affine_dev", "fourq_commit_bytes", "fourq_commit_bytes_dev")


def fixture():
    raw = load_golden("commit.json", raw=True)
    num = lambda P: tuple(tuple(int(c, 16) for c in coord) for coord in P)
    cases = [(c["group_size"], [([int(k, 16) for k in g["k"]], num(g["affine"]), bytes.fromhex(g["enc"])) for g in c["groups"]]) for c in raw["cases"]]
    return [int(t, 16) for t in raw["t"]], [num(B) for B in raw["bases"]], cases


def test_restatement_agrees_with_the_fixture():
    ts, bases, cases = fixture()
    assert len(bases) == 5 and [size for size, _ in cases] == [1, 2, 5, 5] and [len(g) for _, g in cases] == [3, 3, 3, 1]
    for size, groups in cases:
        ks = [k for g in groups for k in g[0]]
        assert ref.commit(ks, bases, size) == [g[1] for g in groups], size
        assert ref.commit_bytes(ks, bases, size) == [g[2] for g in groups], size
    assert cases[-1][1][0][1] == ref.NEUTRAL_AFFINE and cases[-1][1][0][2] == bytes([1] + [0] * 31)
    planted = [k for size, groups in cases[:2] for g in groups for k in g[0]]
    assert {0, 1, o.N - 1, o.N, o.N + 1, (1 << 256) - 1} <= set(planted)


def test_restatement_agrees_with_the_group_law():
    ts, bases, cases = fixture()
    for t, B in zip(ts, bases):
        assert ref.multiple_of_g(t) == B and o.PointOnCurve(B)
    for size, groups in cases:
        for ks, affine, _ in groups:
            assert ref.multiple_of_g(sum(k * t for k, t in zip(ks, ts))) == affine == ref.commit(ks, bases, size)[0]
    ks = [3, 5, 7]
    ks.append(ref.closing_scalar(ks, ts))
    assert ref.commit(ks, bases, 4) == [ref.NEUTRAL_AFFINE]
    assert ref.commit(ks[:3] + [ks[3] ^ 1], bases, 4) != [ref.NEUTRAL_AFFINE]                 # ... and only that scalar closes the sum


def test_header_and_binding_declare_the_same_symbols():
    from fourq_amd import Engine, MultiEngine, _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_commit_\w+)\s*\(([^;{]*)\)\s*;", header))
    assert set(decls) == set(SYMBOLS) == {n for n in _lib.PROTOTYPES if n.startswith("fourq_commit_")}
    arity = {name: len([a for a in args.split(",") if a.strip()]) for name, args in decls.items()}
    for name in SYMBOLS:
        assert arity[name] == len(_lib.PROTOTYPES[name][1]), name
    assert arity == {"fourq_commit_bases_set": 3, "fourq_commit_bases_count": 2, "fourq_commit_route": 1, "fourq_commit_reserve": 3,
                     "fourq_commit_affine": 6, "fourq_commit_affine_dev": 6, "fourq_commit_bytes": 6, "fourq_commit_bytes_dev": 6}
    for host in ("fourq_commit_affine", "fourq_commit_bytes"):
        assert _lib.PROTOTYPES[host] == _lib.PROTOTYPES[host + "_dev"]
        assert re.search(r"size_t\s+groups\s*,\s*size_t\s+group_size\s*,\s*int\s+route\s*$", decls[host]), host
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600
    assert re.search(r"#define\s+FOURQ_COMMIT_MAX_BASES\s+4096\b", header_raw)
    for m in ("commit_bases", "commit_reserve", "commit", "commit_bytes", "commit_dev", "commit_bytes_dev", "commit_generators", "commit_route"):
        assert callable(getattr(Engine, m)), m
    assert isinstance(Engine.commit_bases_count, property)
    for m in ("commit_bases", "commit", "commit_bytes"):
        assert callable(getattr(MultiEngine, m)), m


def test_route_table_and_null_context():
    from fourq_amd import _lib
    lib = _lib.load()
    sizes = sorted(set(range(0, 71)) | {1 << e for e in range(7, 33)} | {(1 << e) + 1 for e in range(7, 32)} | {_lib.MAX_BATCH})
    routes = [lib.fourq_commit_route(s) for s in sizes]
    assert set(routes) <= {1, 2} and routes == sorted(routes, reverse=True)              # gather for few groups, staged from some count on
    assert lib.fourq_commit_reserve(None, 1, 1) == _lib.ERR_INVALID
    assert lib.fourq_commit_bases_set(None, None, 1) == _lib.ERR_INVALID
    assert lib.fourq_commit_bases_count(None, None) == _lib.ERR_INVALID
    for fn in (lib.fourq_commit_affine, lib.fourq_commit_affine_dev, lib.fourq_commit_bytes, lib.fourq_commit_bytes_dev):
        assert fn(None, None, None, 0, 0, 0) == _lib.ERR_INVALID                           # refused before groups == 0 is looked at


# ---- geometry and work buffer ---------------------------------------------------------------------------------------------------------
def a256(n):
    return (n + 255) // 256 * 256


def folded(m):
    return -(-m // 64)


def need(groups, size):
    """bytes each region's pass reads or writes, in carving order: every fold pass's output fits the region it alternates into"""
    first, second = folded(size), folded(folded(size))
    return [("rows", groups * size * 96), ("part_a", groups * first * 96 if size > 1 else 0), ("part_b", groups * second * 96 if first > 1 else 0),
            ("st_zero", groups), ("st_out", groups)]


def geometry(groups, size, blocks_max, width_max):
    """commit_layout.h's comment, restated"""
    n, width = groups * size, 64
    while width < width_max and width < groups and width * blocks_max < n:
        width *= 2
    slices = -(-groups // width)
    return {"width": width, "grid": min(-(-n // width), blocks_max), "slices": slices, "items": slices * size}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("commit_layout") / "commit_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "commit_layout_dump.cpp"), "-o", exe], check=True)

    def run(groups, size, blocks_max=256, width_max=1024):
        out = subprocess.run([exe, str(groups), str(size), str(blocks_max), str(width_max)], check=True, capture_output=True, text=True).stdout
        return {name: int(value) for name, value in (line.split() for line in out.splitlines())}
    return run


DIMS = [1, 2, 3, 63, 64, 65, 130, 255, 256, 257, 1025, 4096, 4097, 65537]


@pytest.mark.parametrize("groups", DIMS)
def test_commit_regions_are_aligned_disjoint_and_never_shrink(layout, groups):
    before = 0
    for size in DIMS:
        if groups * size > 1 << 26:
            continue
        got = layout(groups, size)
        spans = need(groups, size)
        offs = {k[4:]: v for k, v in got.items() if k.startswith("own.")}
        assert list(offs) == [name for name, _ in spans]
        at = 0
        for name, size_bytes in spans:
            assert offs[name] % 16 == 0 and offs[name] >= at, (name, offs[name], at)      # aligned, disjoint, in carving order
            at = offs[name] + size_bytes
        assert at <= got["bytes"] < at + 256
        # the fold's later passes alternate into the same two regions with fewer rows
        m, to_a = size, True
        while m > 1:
            m = folded(m)
            assert groups * m * 96 <= dict(spans)["part_a" if to_a else "part_b"]
            to_a = not to_a
        assert got["bytes"] >= before                                                        # growing group_size never shrinks it
        before = got["bytes"]
        assert layout(groups + 1, size)["bytes"] >= got["bytes"] and layout(groups, size + 1)["bytes"] >= got["bytes"]


@pytest.mark.parametrize("blocks_max,width_max", [(256, 1024), (1024, 256), (8, 1024), (1, 64)])
def test_commit_geometry_tiles_the_items(layout, blocks_max, width_max):
    """The dump program itself checks that the blocks' ranges tile [0, items) in order (exit 3 otherwise)."""
    for groups, size in [(1, 1), (3, 2), (67, 130), (1025, 2), (1025, 3), (2049, 1), (32768, 2), (1024, 64), (64, 1024), (1, 4096), (65536, 1)]:
        got = layout(groups, size, blocks_max, width_max)
        want = geometry(groups, size, blocks_max, width_max)
        assert {k[5:]: v for k, v in got.items() if k.startswith("geom.") and k != "geom.changes"} == want
        assert 64 <= want["width"] <= width_max and want["slices"] * want["width"] >= groups
        assert 1 <= want["grid"] <= min(blocks_max, want["items"])


def test_gpu_shapes_restage_inside_a_block(layout):
    """On a 256-CU chip the GPU tests' shape 67 x 130 gives many blocks an item range that changes base in mid-range -- the path the
    barriers around the staging protect -- in the default mode (one block per CU, up to 1 024 lanes) and in constant-time mode (four
    256-lane blocks per CU) alike.  The width rule keeps 1025 x 2, 1025 x 3 and 2049 x 1 at 64 lanes on such a chip (they hold few rows):
    there every block has one base, and what they check is the second slice of a base and its ragged last block."""
    for blocks_max, width_max in ((256, 1024), (1024, 256)):
        got = layout(67, 130, blocks_max, width_max)
        assert got["geom.changes"] >= 32 and got["geom.slices"] == 2 and got["geom.grid"] == 137          # 61 of the 137 blocks, in fact
        for groups, size in ((1025, 2), (1025, 3), (2049, 1)):
            got = layout(groups, size, blocks_max, width_max)
            assert got["geom.width"] == 64 and got["geom.slices"] == -(-groups // 64) and groups % 64 == 1
    import test_gpu_commit as gpu
    for ct, (blocks_max, width_max) in ((False, (256, 1024)), (True, (1024, 256))):           # ... and blocks of two waves do so here
        groups, size = gpu.WIDE[ct]
        got = layout(groups, size, blocks_max, width_max)
        assert got["geom.width"] == 128 and got["geom.changes"] >= 20 and size == gpu.BASES          # 63 of 133 blocks, 24 of 529
