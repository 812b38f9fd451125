"""The bucket route of the grouped sums before any GPU runs (no GPU needed): the identity it rests on, restated step by step on the Python
oracle (tests/bucket_ref.py) and compared with R1toAffine(sum MUL_endo), what fourq_msm_* computes; the scalar pool the GPU tests use; the
symbols in header and binding; the default-window table; and the work-buffer layout compiled with g++."""
import os
import random
import re
import subprocess

import pytest

import bucket_ref as ref
import curve4q_oracle as o
from conftest import ROOT

WINDOWS = (4, 5, 8, 12)
SIZES = (1, 2, 17, 65)
SYMBOLS = ("fourq_bucketsum_window", "fourq_bucketsum_reserve", "fourq_bucketsum_affine", "fourq_bucketsum_affine_dev", "fourq_bucketsum_bytes",
           "fourq_bucketsum_bytes_dev")

_cache = {}


def points(count):
    """[t]G for seeded t, affine tuples"""
    if "points" not in _cache:
        rng = random.Random(7401)
        G = o.AffineToR1(o.Gx, o.Gy)
        _cache["points"] = [o.R1toAffine(ref.times(rng.getrandbits(40) | 1, G)) for _ in range(max(SIZES))]
    return _cache["points"][:count]


def scalars(count, turn):
    """the six edge scalars and seeded ones, rotated by `turn` so that the short groups see another edge value at every window"""
    rng = random.Random(7402)
    pool = list(ref.EDGE_SCALARS) + [rng.getrandbits(256) for _ in range(max(SIZES))]
    return [pool[(i + turn) % 6] if i < 6 else pool[i] for i in range(count)]


@pytest.mark.parametrize("size", SIZES)
def test_restated_bucket_route_equals_the_sum_of_ladders(size):
    P = points(size)
    for turn, c in enumerate(WINDOWS):
        ks = scalars(size, turn)
        assert ref.bucket_sum(ks, P, c) == ref.ladder_sum(ks, P), (size, c)
    if size == max(SIZES):
        assert set(ref.EDGE_SCALARS) <= set(scalars(size, 0))
        # the comparison has teeth: with phi and psi exchanged in the last step the sums differ
        ks = scalars(2, 0)[4:] + scalars(size, 0)[6:8]
        assert ref.bucket_sum(ks, P[:len(ks)], 4, endo=(o.psi, o.phi)) != ref.ladder_sum(ks, P[:len(ks)])


def test_every_edge_scalar_alone():
    P = points(1)
    for k in ref.EDGE_SCALARS:
        for c in (4, 12):
            assert ref.bucket_sum([k], P, c) == ref.ladder_sum([k], P), (k, c)


def test_endomorphisms_keep_the_neutral():
    for f in (o.phi, o.psi):
        assert ref.is_neutral(f(ref.NEUTRAL))


def test_points_outside_the_subgroup_keep_mul_endos_value():
    """Four decodable strings whose points have [N]P != O: the bucket form still equals the sum of MUL_endo -- which, there, is NOT the sum of
    plain [k]P, so a bucket method over the raw 256-bit scalar could not reproduce the ladder route."""
    found = ref.outside_subgroup_points(7403, 4)
    P = [p for _, p in found]
    for enc, p in found:
        assert o.decode(enc) == p and o.PointOnCurve(p)
        assert not ref.is_neutral(ref.times(o.N, o.AffineToR1(*p)))
    rng = random.Random(7404)
    ks = [rng.getrandbits(256) for _ in P]
    want = ref.ladder_sum(ks, P)
    for c in (4, 8):
        assert ref.bucket_sum(ks, P, c) == want, c
    plain = ref.NEUTRAL
    for k, p in zip(ks, P):
        plain = ref.add(plain, ref.times(k, o.AffineToR1(*p)))
    assert o.R1toAffine(plain) != want


def test_gpu_scalar_pool_reaches_the_digit_edges():
    """For windows 4 and 8 the pool has, in every one of the four sub-scalars, a zero digit (a skipped element) and a maximal one (the
    column's last bucket); and it holds the six edge scalars."""
    import test_gpu_bucket_sum as gpu
    k = ref.pool_scalars(gpu.POOL)
    assert len(k) == gpu.POOL and set(ref.EDGE_SCALARS) <= set(k)
    vs = [ref.sub_scalars(x) for x in k[:2000]]
    for c in (4, 8):
        W = -(-64 // c)
        for j in range(4):
            digits = {ref.digit(v[j], w, c) for v in vs for w in range(W - 1)}      # the full-width windows
            assert 0 in digits and (1 << c) - 1 in digits, (c, j)


def test_header_and_binding_declare_the_same_symbols():
    from fourq_amd import Engine, _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_bucketsum_\w+)\s*\(([^;{]*)\)\s*;", header))
    assert set(decls) == set(SYMBOLS) == {n for n in _lib.PROTOTYPES if "bucketsum" in n}
    arity = {name: len([a for a in args.split(",") if a.strip()]) for name, args in decls.items()}
    for name in SYMBOLS:
        assert arity[name] == len(_lib.PROTOTYPES[name][1]), name
        assert not any(word in name for word in ("msm", "dleq", "oprf", "h2c")) and not name.endswith(("_batch", "_batch_dev"))
    assert arity == {"fourq_bucketsum_window": 1, "fourq_bucketsum_reserve": 4, "fourq_bucketsum_affine": 7, "fourq_bucketsum_affine_dev": 7,
                     "fourq_bucketsum_bytes": 8, "fourq_bucketsum_bytes_dev": 8}
    for host in ("fourq_bucketsum_affine", "fourq_bucketsum_bytes"):
        assert _lib.PROTOTYPES[host] == _lib.PROTOTYPES[host + "_dev"]
        assert re.sub(r"\s+", " ", decls[host]) == re.sub(r"\s+", " ", decls[host + "_dev"])
        assert re.search(r"size_t\s+groups\s*,\s*size_t\s+group_size\s*,\s*unsigned\s+window\s*$", decls[host]), host
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600
    assert "sums across elements: the bucket route" in header_raw
    for m in ("bucket_sum", "bucket_sum_bytes", "bucket_sum_dev", "bucket_sum_bytes_dev", "bucket_sum_reserve", "bucket_sum_window"):
        assert callable(getattr(Engine, m)), m


def test_default_window_is_monotone_and_in_range():
    from fourq_amd import _lib
    lib = _lib.load()
    sizes = sorted(set(range(1, 71)) | {1 << e for e in range(7, 33)} | {(1 << e) + 1 for e in range(7, 32)} | {_lib.MAX_BATCH})
    windows = [lib.fourq_bucketsum_window(s) for s in sizes]
    assert windows[0] == 0 and lib.fourq_bucketsum_window(0) == 0
    assert all(w == 0 or 4 <= w <= 12 for w in windows)
    assert windows == sorted(windows)
    assert lib.fourq_bucketsum_reserve(None, 1, 1, 4) == _lib.ERR_INVALID
    assert lib.fourq_bucketsum_affine(None, None, None, None, 0, 0, 0) == _lib.ERR_INVALID


# ---- the work buffer ------------------------------------------------------------------------------------------------------------------
def a256(n):
    return (n + 255) // 256 * 256


def r4(n):
    return (n + 3) // 4 * 4


def geometry(groups, size, c):
    """bucket_layout.h's comments, restated: W, B, columns, passes, rows per column before each pass, chunks, rows behind the first fold"""
    W, B = -(-64 // c), 1 << c
    passes, reach = 1, 64
    while reach < size:
        passes, reach = passes + 1, reach * 64
    rows = [size]
    for _ in range(6):
        r = rows[-1]
        rows.append(min(r, min(B - 1, r) + r // 64))
    return {"n": groups * size, "windows": W, "digits": B, "cols": groups * 4 * W, "passes": passes, "chunks": B // 16, "fold1": -(-(B // 16) // 64)}, rows


def need(groups, size, c):
    """bytes each region's pass reads or writes, in carving order"""
    g, rows = geometry(groups, size, c)
    n, cols, B = g["n"], g["cols"], g["digits"]
    msm = 2 * n * 160 + a256(n) + n // 2 * 96 + a256(n // 2) + n // 4 * 96 + a256(n // 4)
    return [("inner", msm), ("v", n * 32), ("affine", n * 64), ("st_decode", n), ("group_code", groups * 4), ("counts", cols * B * 4),
            ("off_a", cols * (B + 1) * 4), ("off_b", cols * (B + 1) * 4), ("idx", cols * size * 4), ("rows_a", cols * rows[1] * 96),
            ("rows_b", cols * rows[2] * 96 if g["passes"] > 1 else 0), ("weighted", cols * g["chunks"] * 96),
            ("fold_a", cols * g["fold1"] * 96 if g["chunks"] > 1 else 0), ("fold_b", cols * 96 if g["fold1"] > 1 else 0),
            ("endo", groups * 4 * 96), ("st_endo", groups * 4), ("sum", groups * 96), ("st_sum", groups)]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bucket_layout") / "bucket_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "bucket_layout_dump.cpp"), "-o", exe], check=True)

    def run(groups, size, c):
        out = subprocess.run([exe, str(groups), str(size), str(c)], check=True, capture_output=True, text=True).stdout
        return {name: int(value) for name, value in (line.split() for line in out.splitlines())}
    return run


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 65537])
@pytest.mark.parametrize("c", [4, 8, 12])
def test_bucket_regions_are_aligned_disjoint_and_behind_the_inner_layout(layout, n, c):
    for groups, size in ((1, n), (n, 1)):
        got = layout(groups, size, c)
        g, rows = geometry(groups, size, c)
        assert {k[5:]: v for k, v in got.items() if k.startswith("geom.")} == g
        assert [got["rows.%d" % k] for k in range(7)] == rows
        # every pass's parts fit the rows the next pass may read, whatever the scalars: full parts plus one per non-empty bucket
        for k in range(g["passes"]):
            assert rows[k + 1] >= min(rows[k], min(g["digits"] - 1, rows[k]) + rows[k] // 64)
        worst = size                                                 # one bucket holds the whole group
        for k in range(g["passes"]):
            worst = -(-worst // 64)
        assert worst == 1 and (g["passes"] == 1 or -(-size // 64 ** (g["passes"] - 1)) > 1)
        spans = need(groups, size, c)
        offs = {k[4:]: v for k, v in got.items() if k.startswith("own.")}
        assert list(offs) == [name for name, _ in spans]                                    # the dump lists them in carving order
        assert offs["inner"] == 0 and offs["v"] >= got["inner_bytes"] == spans[0][1]       # behind the inner layout
        at = 0
        for name, size_bytes in spans:
            assert offs[name] % 16 == 0 and offs[name] >= at, (name, offs[name], at)      # aligned, disjoint, in carving order
            at = offs[name] + size_bytes
        assert at <= got["bytes"] < at + 256                                               # ... and the last one ends at bytes()
        assert got["zeroed_bytes"] == offs["off_a"] - offs["group_code"] >= spans[4][1] + spans[5][1]
        assert offs["counts"] + spans[5][1] == offs["off_a"]                               # one memset covers group_code and counts
