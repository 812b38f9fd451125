"""The oblivious PRF on the CPU (no GPU needed): the restatement (tests/oprf_ref.py) against the rows the real reference's point functions
produced (tests/golden/oprf.json), the protocol identity finalize(blind, evaluate) == eval, what the fixture promises to cover, the
header against the binding, and the four work-buffer layouts compiled with g++."""
import os
import re
import subprocess

import pytest

import oprf_ref as ref
import ref_loader
from conftest import GOLDEN, ROOT

N = ref.N
TOP = (1 << 256) - 1


def rows(golden):
    return golden("oprf.json", raw=True)["rows"]


def fields(c):
    return bytes.fromhex(c["dst"]), bytes.fromhex(c["msg"]), int(c["r"], 16), int(c["key"], 16)


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_oprf", os.path.join(GOLDEN, "make_oprf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "oprf.json")) as fh:
        assert mod.generate() == fh.read()


def test_fixture_covers_the_cases_it_promises(golden):
    cases = rows(golden)
    assert os.path.getsize(os.path.join(GOLDEN, "oprf.json")) < 64 * 1024
    assert 14 <= len(cases) <= 20
    assert {len(c["dst"]) // 2 for c in cases} == {1, 255}
    assert {1, N - 1, N + 1, TOP} <= {int(c["r"], 16) for c in cases}
    assert {1, N - 1, TOP} <= {int(c["key"], 16) for c in cases}
    for dl in (1, 255):
        # F's string is 32 + len + (8 + dl + 1) bytes: both sides of "marker and length still fit the block" (111 | 112 mod 128) and of
        # "the string fills the block" (127 | 128 | 129 mod 128)
        totals = {32 + len(c["msg"]) // 2 + 9 + dl for c in cases if len(c["dst"]) // 2 == dl}
        assert 32 + 9 + dl in totals                                            # the empty message
        assert {110, 111, 112, 127, 0, 1} <= {t % 128 for t in totals}


def test_restatement_reproduces_the_golden_rows(golden):
    for c in rows(golden):
        dst, msg, r, key = fields(c)
        blinded, st = ref.blind(msg, dst, r)
        assert (blinded.hex(), st) == (c["blinded"], 0)
        evaluated, st = ref.evaluate(key, blinded)
        assert (evaluated.hex(), st) == (c["evaluated"], 0)
        out, st = ref.finalize(msg, dst, r, evaluated)
        assert (out.hex(), st) == (c["output"], 0)
        assert ref.final_hash(bytes.fromhex(c["unblinded"]), msg, dst).hex() == c["output"]


def test_finalize_of_blind_and_evaluate_is_the_direct_evaluation(golden):
    for c in rows(golden):
        dst, msg, r, key = fields(c)
        assert ref.evaluate_direct(key, msg, dst) == (bytes.fromhex(c["output"]), 0)
        # ... and for a blind the fixture does not hold: the output does not depend on it
        other = (r * 3 + 5) % N or 7
        blinded, _ = ref.blind(msg, dst, other)
        assert ref.finalize(msg, dst, other, ref.evaluate(key, blinded)[0]) == (bytes.fromhex(c["output"]), 0)


def test_restatement_reports_bad_rows_as_the_header_says():
    assert ref.blind(b"m", b"d", 0) == (bytes(32), ref.BLIND_ZERO) and ref.blind(b"m", b"d", 2 * N) == (bytes(32), ref.BLIND_ZERO)
    good, _ = ref.blind(b"m", b"d", 5)
    assert ref.finalize(b"m", b"d", N, good) == (bytes(64), ref.BLIND_ZERO)
    neutral = bytes([1] + [0] * 31)                                                 # decode refuses it (the reference's t == 0 branch)
    assert ref.finalize(b"m", b"d", 0, neutral) == (bytes(64), 16 + 3)              # decode takes precedence over the zero blind
    assert ref.evaluate(7, neutral) == (bytes(32), 16 + 3)
    assert ref.evaluate(N, good) == (bytes(32), ref.DH_NEUTRAL) and ref.evaluate_direct(0, b"m", b"d") == (bytes(64), ref.DH_NEUTRAL)
    # F is injective in (E, msg, dst): moving a byte between the fields changes the string
    assert ref.final_hash(bytes(32), b"ab", b"c") != ref.final_hash(bytes(32), b"a", b"bc")


def test_header_and_binding_declare_the_same_new_symbols():
    from fourq_amd import _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_(?:oprf|scalar_inv)_\w+)\s*\(([^;{]*)\)\s*;", header))
    arity = {"fourq_oprf_blind_batch": 11, "fourq_oprf_evaluate_batch": 6, "fourq_oprf_finalize_batch": 12, "fourq_oprf_eval_batch": 11, "fourq_scalar_inv_batch": 4}
    new = set(arity) | {n + "_dev" for n in arity}
    assert set(decls) == new == {n for n in _lib.PROTOTYPES if "oprf" in n or "scalar_inv" in n}
    for name, args in decls.items():
        count = len([a for a in args.split(",") if a.strip()])
        assert count == len(_lib.PROTOTYPES[name][1]) == arity[name.replace("_dev", "")], name
        assert _lib.PROTOTYPES[name][1] == _lib.PROTOTYPES[name.replace("_dev", "")][1], name
    # the message arguments are those of fourq_sha512_batch, behind dst and dst_len
    sha = _lib.PROTOTYPES["fourq_sha512_batch"][1]
    for name, at in (("fourq_oprf_blind_batch", 3), ("fourq_oprf_finalize_batch", 3), ("fourq_oprf_eval_batch", 4)):
        assert _lib.PROTOTYPES[name][1][at:at + 4] == sha[1:5], name
    # the one test hook of the feature is a call behind FOURQ_DEBUG_ROUTES, not a variable: the set of variables the library reads is pinned
    assert re.search(r"\bint\s+fourq_ctx_set_scinv_group\s*\(\s*fourq_ctx\s*\*\s*ctx\s*,\s*int\s+k\s*\)\s*;", header) and len(_lib.PROTOTYPES["fourq_ctx_set_scinv_group"][1]) == 2
    assert re.search(r"#define\s+FOURQ_OPRF_BLIND_ZERO\s+48\b", header) and _lib.OPRF_BLIND_ZERO == 48 == ref.BLIND_ZERO
    assert re.search(r"FOURQ_SC_INV\s*=\s*71\b", header) and _lib.PRIM["SC_INV"] == 71
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600
    from fourq_amd import Engine, MultiEngine
    protocol = ("oprf_blind", "oprf_evaluate", "oprf_finalize", "oprf_eval")
    assert all(callable(getattr(Engine, m)) and callable(getattr(Engine, m + "_dev")) for m in protocol + ("scalar_inv",))
    assert all(callable(getattr(MultiEngine, m)) for m in protocol)


def test_bytes_module_carries_a_known_answer_the_restatement_confirms():
    from fourq_amd import oprf
    r, key = oprf.KAT_BLIND, oprf.KAT_KEY
    blinded, st = ref.blind(oprf.KAT_MSG, oprf.KAT_DST, r)
    assert (blinded.hex(), st) == (oprf.KAT_BLINDED, 0)
    evaluated, st = ref.evaluate(key, blinded)
    assert (evaluated.hex(), st) == (oprf.KAT_EVALUATED, 0)
    assert ref.finalize(oprf.KAT_MSG, oprf.KAT_DST, r, evaluated) == (bytes.fromhex(oprf.KAT_OUTPUT), 0)
    assert ref.evaluate_direct(key, oprf.KAT_MSG, oprf.KAT_DST) == (bytes.fromhex(oprf.KAT_OUTPUT), 0)


# ---- the work-buffer layouts (work_layout.h), compiled with g++ ----------------------------------------------------------------------
def a(n):
    return (n + 255) & ~255


# region -> bytes, in the order the header carves them; u lies ON another region and is checked apart
NEED = {
    "blind": {"pts": lambda n: 64 * n, "rows_in": lambda n: 160 * n, "rows_out": lambda n: 160 * n, "st_decode": a},
    "evaluate": {"dh": lambda n: 128 * n + 2 * a(n), "keys": lambda n: 32 * n},
    "finalize": {"inv": lambda n: 32 * n, "rows_in": lambda n: 160 * n, "rows_out": lambda n: 160 * n, "e32": lambda n: 32 * n, "st_decode": a, "st_lower": a, "st_zero": a},
    "eval": {"pts": lambda n: 64 * n, "shared": lambda n: 64 * n, "keys": lambda n: 32 * n, "e32": lambda n: 32 * n, "st_dh": a},
}
ALIAS = {"blind": ("u", "rows_in"), "eval": ("u", "shared")}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("oprf_layout") / "oprf_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "oprf_layout_dump.cpp"), "-o", exe], check=True)

    def run(n):
        return {name: int(value) for name, value in (line.split() for line in subprocess.run([exe, str(n)], check=True, capture_output=True, text=True).stdout.splitlines())}
    return run


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537, 0xffffff00])
def test_oprf_regions_are_aligned_disjoint_and_end_at_the_total(layout, n):
    offs = layout(n)
    sig_verify, dh_bytes = offs.pop("sig_verify_bytes"), offs.pop("dh_bytes_bytes")
    assert dh_bytes == NEED["evaluate"]["dh"](n)
    # what a layout admits for the calls its call makes (work_layout.h, the rule): evaluate calls DH_endo on encodings over n rows (restated
    # from fourq_amd.hip), which carves DhBytes; the other three make no call with a layout of its own
    extent = {call: offs.pop(call + "_inner_extent") for call in NEED}
    assert extent == {"blind": 0, "evaluate": offs["evaluate.keys"], "finalize": 0, "eval": 0} and extent["evaluate"] >= dh_bytes
    for call, need in NEED.items():
        mine = {k.split(".")[1]: v for k, v in offs.items() if k.startswith(call + ".")}
        total = mine.pop("bytes")
        if call in ALIAS:
            alias, host = ALIAS[call]
            assert mine.pop(alias) == mine[host] and 64 * n <= need[host](n)         # u (n x 8 words) lies on a region that holds it
        assert list(mine) == list(need)
        spans = sorted((off, off + need[name](n), name) for name, off in mine.items())
        assert spans[0][0] == 0 and [name for _, _, name in spans] == list(need)    # carved in the order the header lists them
        for off, end, name in spans:
            assert off % 16 == 0 and end <= total, (call, name, off, end, total)
        for (_, end, name), (off, _, nxt) in zip(spans, spans[1:]):
            assert end <= off, (call, name, nxt)
        assert spans[-1][1] == total == sum(f(n) for f in need.values()), call
        # fourq_ctx_reserve takes the maximum over the layouts: these stay below the signature check's, so reserve does not grow
        assert total <= sig_verify == 2 * n * 160 + 3 * a(n) + 3 * n * 32, call
