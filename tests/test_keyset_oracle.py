"""Signatures of registered keys before any GPU runs (no GPU needed): the restatement on the Python oracle (tests/keyset_ref.py) against the
fixture made with the reference's point functions (tests/golden/keyset.json) and against sig_ref; the order check; the symbols in header
and binding; and the work-buffer layout (fourq_amd/csrc/keyset_layout.h) compiled with g++."""
import os
import re
import subprocess

import pytest

import curve4q_oracle as o
import keyset_ref as ref
import sig_ref
from conftest import ROOT, load_golden

SYMBOLS = ("fourq_keyset_set", "fourq_keyset_count", "fourq_keyset_reserve", "fourq_keyset_double_mul_bytes", "fourq_keyset_double_mul_bytes_dev",
           "fourq_keyset_sig_verify", "fourq_keyset_sig_verify_dev")
EDGES = [0, 1, 2, o.N - 1, o.N, o.N + 1, (1 << 256) - 1]


def fixture():
    raw = load_golden("keyset.json", raw=True)
    keys = [bytes.fromhex(k["pk"]) for k in raw["keys"]]
    statuses = [k["status"] for k in raw["keys"]]
    rows = [(r["_how"], r["id"], bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["ok"], r["status"]) for r in raw["rows"]]
    scalar_rows = [(r["id"], int(r["k"], 16), int(r["l"], 16), bytes.fromhex(r["out"]), r["status"]) for r in raw["scalar_rows"]]
    return keys, statuses, rows, scalar_rows


def test_key_statuses_agree_with_the_fixture():
    keys, statuses, _, _ = fixture()
    assert len(keys) == 5
    assert [ref.key_status(pk) for pk in keys] == statuses
    assert statuses == [0, 0, 0, sig_ref.BYTES_DECODE_BASE + sig_ref.DECODE_NOT_ON_CURVE, ref.KEYSET_NOT_ORDER_N]


def test_the_negated_key_is_on_the_curve_and_outside_the_subgroup():
    keys, _, _, _ = fixture()
    A, B = o.decode(keys[0]), o.decode(keys[4])
    p = (1 << 127) - 1
    assert [[(-int(c)) % p for c in coord] for coord in A] == [[int(c) for c in coord] for coord in B]          # (-x, -y)
    assert o.PointOnCurve(B)
    assert ref.plain_mul(o.N, A) == ref.NEUTRAL_AFFINE                                      # an honest key has order N ...
    assert ref.plain_mul(o.N, B) == ((0, 0), (p - 1, 0))                                    # ... A + (0, -1) has order 2N: [N] of it is (0, -1)
    assert ref.plain_mul(2 * o.N, B) == ref.NEUTRAL_AFFINE
    assert ref.plain_mul(o.N, (o.Gx, o.Gy)) == ref.NEUTRAL_AFFINE
    # plain_mul is [k]P where MUL_endo is: on the subgroup
    assert ref.plain_mul(12345, A) == tuple(tuple(int(c) for c in coord) for coord in o.R1toAffine(o.MUL_endo(12345, o.AffineToR1(*A))))


def test_verify_rows_agree_with_the_fixture_and_with_sig_ref():
    keys, statuses, rows, _ = fixture()
    assert 20 <= len(rows) <= 30
    hows = {how.split(":")[0] for how, *_ in rows}
    assert {"valid", "msg bit", "R bit", "s bit", "s + N", "length one short", "pk bit", "pk off curve", "s = N"} <= hows
    for how, kid, msg, sig, ok, st in rows:
        assert ref.verify_keyed(keys, kid, msg, sig) == (ok, st), how
        if statuses[kid] == 0:
            assert sig_ref.verify(keys[kid], msg, sig) == (ok, st), how                     # an accepted key: the unkeyed call's answer
        else:
            assert (ok, st) == (0, statuses[kid]), how                                      # the key's status wins over s >= N
    assert any(sig_ref.LE(sig[32:]) == o.N and st == ref.SIG_S_RANGE for _, _, _, sig, _, st in rows)
    assert ref.verify_keyed(keys, len(keys), rows[0][2], rows[0][3]) == (0, ref.KEYSET_ID_RANGE)


def test_scalar_rows_agree_with_the_fixture():
    keys, statuses, _, scalar_rows = fixture()
    assert {(k, l) for _, k, l, _, _ in scalar_rows} >= {(k, l) for k in EDGES for l in EDGES}      # every pair of parities among them
    for kid, k, l, out, st in scalar_rows:
        assert ref.double_mul_keyed(keys, kid, k, l) == (out, st), (kid, hex(k), hex(l))
        assert (st == 0) == (statuses[kid] == 0) and (st != 0) == (out == ref.ZERO_ROW)
    assert scalar_rows[0][1:4] == (0, 0, ref.NEUTRAL_BYTES)
    assert ref.double_mul_keyed(keys, 7, 1, 1) == (ref.ZERO_ROW, ref.KEYSET_ID_RANGE)


def test_header_and_binding_declare_the_same_symbols():
    from fourq_amd import Engine, MultiEngine, _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_keyset_\w+)\s*\(([^;{]*)\)\s*;", header))
    assert set(decls) == set(SYMBOLS) == {n for n in _lib.PROTOTYPES if n.startswith("fourq_keyset_")}
    arity = {name: len([a for a in args.split(",") if a.strip()]) for name, args in decls.items()}
    for name in SYMBOLS:
        assert arity[name] == len(_lib.PROTOTYPES[name][1]), name
    assert arity == {"fourq_keyset_set": 4, "fourq_keyset_count": 2, "fourq_keyset_reserve": 2, "fourq_keyset_double_mul_bytes": 8,
                     "fourq_keyset_double_mul_bytes_dev": 8, "fourq_keyset_sig_verify": 11, "fourq_keyset_sig_verify_dev": 11}
    # the two new status codes collide with no status byte the header defines
    codes = {name: int(v, 0) for name, v in re.findall(r"#define\s+(FOURQ_(?:DH|DECODE|SIG|OPRF|DLEQ|KEYSET)_[A-Z_0-9]+)\s+(\d+)\b", header_raw)
             if not name.endswith(("MAX_MSG", "MAX_KEYS"))}
    base = int(re.search(r"#define\s+FOURQ_BYTES_DECODE_BASE\s+(\d+)", header_raw).group(1))
    taken = {v for n, v in codes.items() if not n.startswith("FOURQ_KEYSET_") and not n.startswith("FOURQ_DECODE_")}
    taken |= {base + v for n, v in codes.items() if n.startswith("FOURQ_DECODE_")}
    assert codes["FOURQ_KEYSET_NOT_ORDER_N"] == _lib.KEYSET_NOT_ORDER_N == ref.KEYSET_NOT_ORDER_N
    assert codes["FOURQ_KEYSET_ID_RANGE"] == _lib.KEYSET_ID_RANGE == ref.KEYSET_ID_RANGE
    assert not {_lib.KEYSET_NOT_ORDER_N, _lib.KEYSET_ID_RANGE} & taken and _lib.KEYSET_NOT_ORDER_N != _lib.KEYSET_ID_RANGE
    assert re.search(r"#define\s+FOURQ_KEYSET_MAX_KEYS\s+4096\b", header_raw) and _lib.KEYSET_MAX_KEYS == 4096
    for m in ("keyset_set", "keyset_count", "keyset_reserve", "keyset_double_mul_bytes", "keyset_double_mul_bytes_dev", "sig_verify_keyed", "sig_verify_keyed_dev"):
        assert callable(getattr(Engine, m)), m
    for m in ("keyset_set", "keyset_count", "keyset_double_mul_bytes", "sig_verify_keyed"):
        assert callable(getattr(MultiEngine, m)), m


def test_null_context_is_refused_first():
    from fourq_amd import _lib
    lib = _lib.load()
    assert lib.fourq_keyset_set(None, None, 1, None) == _lib.ERR_INVALID
    assert lib.fourq_keyset_count(None, None) == _lib.ERR_INVALID
    assert lib.fourq_keyset_reserve(None, 0) == _lib.ERR_INVALID
    for fn in (lib.fourq_keyset_double_mul_bytes, lib.fourq_keyset_double_mul_bytes_dev):
        assert fn(None, None, None, None, None, None, None, 0) == _lib.ERR_INVALID          # refused before n == 0 is looked at
    for fn in (lib.fourq_keyset_sig_verify, lib.fourq_keyset_sig_verify_dev):
        assert fn(None, None, None, None, 0, None, 0, None, None, None, 0) == _lib.ERR_INVALID


# ---- work buffer ----------------------------------------------------------------------------------------------------------------------
def a256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("keyset_layout") / "keyset_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "keyset_layout_dump.cpp"), "-o", exe], check=True)

    def run(n):
        out = subprocess.run([exe, str(n)], check=True, capture_output=True, text=True).stdout
        return {name: int(value) for name, value in (line.split() for line in out.splitlines())}
    return run


def test_keyset_regions_are_aligned_disjoint_and_never_shrink(layout):
    before = 0
    for n in [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 4097, 65536, 65537, 1 << 20, (1 << 20) + 1]:
        got = layout(n)
        # bytes each region's kernel reads or writes, in carving order; `inner` is what the existing routes ask for themselves
        spans = [("inner", got["inner"]), ("s", 32 * n), ("h", 32 * n), ("r32", 32 * n), ("rows", 96 * n), ("pk32", 32 * n), ("pre", n)]
        offs = {k[4:]: v for k, v in got.items() if k.startswith("own.")}
        assert list(offs) == [name for name, _ in spans]
        assert offs["inner"] == 0                                                            # the existing routes carve from the first byte
        at = 0
        for name, size_bytes in spans:
            assert offs[name] % 16 == 0 and offs[name] >= at, (name, offs[name], at)       # aligned, disjoint, in carving order
            at = offs[name] + size_bytes
        assert at <= got["bytes"] < at + 256
        assert got["inner"] >= 416 * n and got["inner"] < got["bytes"]
        assert got["bytes"] >= before
        before = got["bytes"]
        assert layout(n + 1)["bytes"] >= got["bytes"]
        # what the layout admits for its inner calls (work_layout.h, the rule) is the offset of its first own region.  Restated from
        # fourq_amd.hip, the constant-time routes call [k]B + [l]P over n rows, and the signature check over n rows, which calls it in turn
        # within ITS inner extent: the double multiplication's layout without the tail it lends the signature check
        assert got["inner_extent"] == offs["s"]
        assert got["inner_extent"] >= got["inner"] and got["inner_extent"] >= got["sig_verify.bytes"]
        assert got["sig_verify.inner_extent"] >= got["inner"] - got["double_mul.lent"] == 320 * n + 2 * a256(n)
