"""The batched DLEQ proofs on the CPU (no GPU needed): the restatement (tests/dleq_ref.py) against the groups the real reference's point
functions produced (tests/golden/dleq.json), completeness for every nonce that is not 0 mod N, the soundness list, the statuses, the header
against the binding, and the work-buffer layout (dleq_layout.h) compiled with g++."""
import functools
import os
import re
import subprocess

import pytest

import dleq_ref as ref
import oprf_ref
import ref_loader
from conftest import GOLDEN, ROOT, load_golden

N = ref.N
TOP = (1 << 256) - 1
DST_LENGTHS = {1, 2, 69, 70, 129, 130, 197, 198, 255}


def cases():
    return load_golden("dleq.json", raw=True)["cases"]


def fields(c):
    return bytes.fromhex(c["dst"]), int(c["key"], 16), bytes.fromhex(c["pk"]), c["group_size"]


def rows(g):
    return [bytes.fromhex(b) for b in g["blinded"]], [bytes.fromhex(b) for b in g["evaluated"]]


@functools.lru_cache(maxsize=None)
def honest():
    """the fixture's first case of two groups of two rows, flattened: key, pk, blinded, evaluated, proofs, dst, group_size"""
    c = next(c for c in cases() if c["group_size"] == 2 and len(c["groups"]) == 2)
    dst, key, pk, group_size = fields(c)
    blinded = [b for g in c["groups"] for b in rows(g)[0]]
    evaluated = [b for g in c["groups"] for b in rows(g)[1]]
    return key, pk, blinded, evaluated, [bytes.fromhex(g["proof"]) for g in c["groups"]], dst, group_size


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dleq", os.path.join(GOLDEN, "make_dleq.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "dleq.json")) as fh:
        assert mod.generate() == fh.read()


def test_fixture_covers_the_cases_it_promises():
    cs = cases()
    assert os.path.getsize(os.path.join(GOLDEN, "dleq.json")) < 64 * 1024
    assert 24 <= sum(len(c["groups"]) for c in cs) <= 60                                  # a few dozen groups
    assert {c["group_size"] for c in cs} == {1, 2, 3, 65}
    assert {len(c["dst"]) // 2 for c in cs} == DST_LENGTHS
    for ln in DST_LENGTHS:
        assert {c["group_size"] for c in cs if len(c["dst"]) // 2 == ln} >= {1, 2, 3}
    # the lengths sit on both sides of every block edge of the two strings: L bytes take ceil((L + 17) / 128) blocks
    blocks = lambda total: (total + 17 + 127) // 128
    assert [blocks(110 + ln) for ln in sorted(DST_LENGTHS)] == [1, 2, 2, 2, 2, 3, 3, 3, 3]
    assert [blocks(170 + ln) for ln in sorted(DST_LENGTHS)] == [2, 2, 2, 3, 3, 3, 3, 4, 4]
    assert {1, N - 1, TOP} <= {int(c["key"], 16) for c in cs}
    assert {1, N - 1, N + 1, TOP} <= {int(g["nonce"], 16) for c in cs for g in c["groups"]}
    for c in cs:
        for g in c["groups"]:
            assert len(g["blinded"]) == len(g["evaluated"]) == len(g["d"]) == c["group_size"]
            assert len(g["M32"]) == len(g["Z32"]) == 64 and len(g["proof"]) == 128


def test_restatement_reproduces_the_golden_groups():
    for c in cases():
        dst, key, pk, _ = fields(c)
        assert ref.public_key(key) == (pk, 0)
        for g in c["groups"]:
            cs, ds = rows(g)
            proof, st, parts = ref.prove_group(key, cs, ds, int(g["nonce"], 16), dst, parts=True)
            assert (proof.hex(), st) == (g["proof"], 0)
            assert ["%x" % d for d in parts["d"]] == g["d"] and parts["M32"].hex() == g["M32"] and parts["Z32"].hex() == g["Z32"]
            # the prover's Z = DH_endo(k, M) is the verifier's sum over the evaluated rows
            assert ref.composites_group(pk, cs, ds, dst) == (parts["M32"], parts["Z32"], 0)
            assert ref.verify_group(pk, cs, ds, proof, dst) == (1, 0)


def test_every_nonce_that_is_not_zero_mod_n_gives_a_proof_that_verifies():
    key, pk, blinded, evaluated, _, dst, group_size = honest()
    cs, ds = blinded[:group_size], evaluated[:group_size]
    seen = set()
    for nonce in (1, 2, N - 1, N + 1, 2 * N - 2, TOP, 0x1234567890ABCDEF << 180):
        proof, st = ref.prove_group(key, cs, ds, nonce, dst)
        assert st == 0 and ref.verify_group(pk, cs, ds, proof, dst) == (1, 0), hex(nonce)
        seen.add(proof)
    assert len(seen) == 6                                                               # 1 and N + 1 are the same nonce
    for nonce in (0, N, 2 * N):
        assert ref.prove_group(key, cs, ds, nonce, dst) == (bytes(64), ref.NONCE_ZERO)


def test_soundness_every_tampering_is_refused_with_status_zero():
    key, pk, blinded, evaluated, proofs, dst, group_size = honest()
    assert ref.verify(pk, blinded, evaluated, proofs, dst, group_size) == [(1, 0), (1, 0)]
    labels = []
    for label, pk_t, b, e, p, dst_t, failing in ref.soundness_cases(key, pk, blinded, evaluated, proofs, dst, group_size):
        got = ref.verify(pk_t, b, e, p, dst_t, group_size)
        assert got == [(0 if g in failing else 1, 0) for g in range(len(proofs))], label
        labels.append(label)
    assert len(labels) == 7 and {"one flipped bit in " + w for w in ("c", "s", "pk", "dst")} <= set(labels)


def test_a_second_encoding_of_s_or_c_is_out_of_range():
    key, pk, blinded, evaluated, proofs, dst, group_size = honest()
    cs, ds, proof = blinded[:group_size], evaluated[:group_size], proofs[0]
    c, s = int.from_bytes(proof[:32], "little"), int.from_bytes(proof[32:], "little")
    assert s + N < 1 << 256 and c + N < 1 << 256                                         # both still fit 32 bytes
    assert ref.verify_group(pk, cs, ds, proof[:32] + (s + N).to_bytes(32, "little"), dst) == (0, ref.SIG_S_RANGE)
    assert ref.verify_group(pk, cs, ds, (c + N).to_bytes(32, "little") + proof[32:], dst) == (0, ref.SIG_S_RANGE)


def test_restatement_reports_bad_groups_as_the_header_says():
    key, pk, blinded, evaluated, proofs, dst, group_size = honest()
    cs, ds, proof = blinded[:group_size], evaluated[:group_size], proofs[0]
    not_on_curve = bytes([2] + [0] * 31)
    assert oprf_ref.decode_status(not_on_curve)[1] == oprf_ref.DECODE_NOT_ON_CURVE and oprf_ref.decode_status(ref.NEUTRAL32)[1] == 3
    # prove: a C row that does not decode; the largest code of the group; a D row that does not decode is only hashed
    assert ref.prove_group(key, [cs[0], not_on_curve], ds, 5, dst) == (bytes(64), 16 + 2)
    assert ref.prove_group(key, [ref.NEUTRAL32, not_on_curve], ds, 5, dst) == (bytes(64), 16 + 3)
    assert ref.prove_group(key, cs, [ds[0], not_on_curve], 5, dst)[1] == 0
    assert ref.prove_group(N, cs, ds, 5, dst) == (bytes(64), ref.DH_NEUTRAL) and ref.prove_group(N, cs, ds, 0, dst) == (bytes(64), ref.DH_NEUTRAL)
    assert ref.prove_group(N, [cs[0], not_on_curve], ds, 0, dst) == (bytes(64), 16 + 2)            # decode first, then the key, then the nonce
    # verify: C, D and pk all count; the range comes behind them
    assert ref.verify_group(pk, [cs[0], not_on_curve], ds, proof, dst) == (0, 16 + 2)
    assert ref.verify_group(pk, cs, [ref.NEUTRAL32, ds[1]], proof, dst) == (0, 16 + 3)
    assert ref.verify_group(not_on_curve, cs, ds, proof, dst) == (0, 16 + 2)
    out_of_range = proof[:32] + bytes([255] * 32)
    assert ref.verify_group(pk, cs, ds, out_of_range, dst) == (0, ref.SIG_S_RANGE) and ref.verify_group(not_on_curve, cs, ds, out_of_range, dst) == (0, 16 + 2)
    assert ref.composites_group(pk, [cs[0], not_on_curve], ds, dst) == (bytes(32), bytes(32), 16 + 2)
    # d depends on the row's index inside the group, not on the group's place in the batch
    assert ref.composite_scalar(pk, cs[0], ds[0], 0, dst) != ref.composite_scalar(pk, cs[0], ds[0], 1, dst)
    assert ref.prove(key, blinded, evaluated, [7, 9], dst, group_size)[1] == ref.prove_group(key, blinded[group_size:], evaluated[group_size:], 9, dst)


def test_header_and_binding_declare_the_same_new_symbols():
    from fourq_amd import _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_dleq_\w+)\s*\(([^;{]*)\)\s*;", header))
    arity = {"fourq_dleq_composites": 11, "fourq_dleq_prove": 12, "fourq_dleq_verify": 12}
    new = set(arity) | {n + "_dev" for n in arity} | {"fourq_dleq_reserve"}
    assert set(decls) == new == {n for n in _lib.PROTOTYPES if "dleq" in n}
    for name, args in decls.items():
        count = len([a for a in args.split(",") if a.strip()])
        assert count == len(_lib.PROTOTYPES[name][1]) == (3 if name == "fourq_dleq_reserve" else arity[name.replace("_dev", "")]), name
        assert _lib.PROTOTYPES[name][1] == _lib.PROTOTYPES[name.replace("_dev", "")][1], name
    assert re.search(r"#define\s+FOURQ_DLEQ_NONCE_ZERO\s+80\b", header) and _lib.DLEQ_NONCE_ZERO == 80 == ref.NONCE_ZERO
    assert "oblivious PRF: proofs" in header_raw
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600      # functions were added, no struct changed
    from fourq_amd import Engine, MultiEngine
    calls = ("dleq_composites", "dleq_prove", "dleq_verify")
    assert all(callable(getattr(Engine, m)) and callable(getattr(Engine, m + "_dev")) for m in calls)
    assert callable(Engine.dleq_reserve) and callable(Engine.dleq_public_key)
    assert callable(MultiEngine.dleq_prove) and callable(MultiEngine.dleq_verify)


def test_bytes_module_carries_a_known_answer_the_restatement_confirms():
    from fourq_amd import oprf
    assert all(callable(getattr(oprf, f)) for f in ("public_key", "prove", "verify"))
    pk, st = ref.public_key(oprf.KAT_KEY)
    assert (pk.hex(), st) == (oprf.KAT_PK, 0)
    blinded, evaluated = bytes.fromhex(oprf.KAT_BLINDED), bytes.fromhex(oprf.KAT_EVALUATED)
    assert oprf_ref.evaluate(oprf.KAT_KEY, blinded) == (evaluated, 0)
    proof, st = ref.prove_group(oprf.KAT_KEY, [blinded], [evaluated], oprf.KAT_NONCE, oprf.KAT_DST)
    assert (proof.hex(), st) == (oprf.KAT_PROOF, 0)
    assert ref.verify_group(pk, [blinded], [evaluated], proof, oprf.KAT_DST) == (1, 0)


# ---- the work-buffer layout (dleq_layout.h), compiled with g++ ---------------------------------------------------------------------------
def a(n):
    return (n + 255) & ~255


# own region -> bytes, in the order the header carves them behind `inner`
OWN = {
    "d": lambda n, g: 32 * n, "pk": lambda n, g: 32 * g, "m32": lambda n, g: 32 * g, "z32": lambda n, g: 32 * g, "t2": lambda n, g: 32 * (g + 1), "t3": lambda n, g: 32 * g,
    "sc_a": lambda n, g: 32 * (g + 1), "sc_b": lambda n, g: 32 * g, "pair_sc": lambda n, g: 64 * g, "pair_pt": lambda n, g: 64 * g, "affine": lambda n, g: 64 * (g + 1),
    "st_m": lambda n, g: a(g), "st_z": lambda n, g: a(g), "st_t2": lambda n, g: a(g + 1), "st_t3": lambda n, g: a(g), "st_pre": lambda n, g: a(g),
}
# what each inner call's layout takes at the size it is called with, from work_layout.h's structs as tests/test_work_layout.py pins them
INNER = {
    "msm_rows": lambda n, g: 320 * n + a(n) + 96 * (n // 2) + a(n // 2) + 96 * (n // 4) + a(n // 4),
    "msm_pair": lambda n, g: 320 * 2 * g + a(2 * g) + 96 * g + a(g) + 96 * (g // 2) + a(g // 2),
    "double_mul": lambda n, g: 320 * g + 2 * a(g) + 96 * g + a(g),
    "evaluate": lambda n, g: 128 * g + 2 * a(g) + 32 * g,
    "mul_rows": lambda n, g: 384 * g + a(g),
    "sig": lambda n, g: 160 * (g + 1) + a(g + 1),
}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dleq_layout") / "dleq_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "dleq_layout_dump.cpp"), "-o", exe], check=True)

    def run(n, groups):
        out = subprocess.run([exe, str(n), str(groups)], check=True, capture_output=True, text=True).stdout
        return {name: int(value) for name, value in (line.split() for line in out.splitlines())}
    return run


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4095, 65537, 0xffffff00])
@pytest.mark.parametrize("one_group", [True, False], ids=["one-group", "groups-of-one"])
def test_dleq_regions_are_aligned_disjoint_behind_the_inner_layouts_and_end_at_the_total(layout, n, one_group):
    groups = 1 if one_group else n
    offs = layout(n, groups)
    total, inner_bytes, plane_rows, inner_extent = offs.pop("bytes"), offs.pop("inner_bytes"), offs.pop("plane_rows"), offs.pop("inner_extent")
    inner = {k.split(".")[1]: v for k, v in offs.items() if k.startswith("inner.")}
    own = {k.split(".")[1]: v for k, v in offs.items() if k.startswith("own.")}
    assert own.pop("inner") == 0
    # the inner calls' own layouts, at the sizes they are called with: the header's numbers are the ones worked out from work_layout.h
    assert inner == {name: f(n, groups) for name, f in INNER.items()}
    assert inner_bytes == max(inner.values())
    assert list(own) == list(OWN)
    spans = [(off, off + OWN[name](n, groups), name) for name, off in own.items()]
    assert spans == sorted(spans)                                                       # carved in the order the header lists them
    assert spans[0][0] == inner_bytes                                                   # the own regions start behind the largest inner layout ...
    for off, end, name in spans:
        assert off % 16 == 0 and off >= max(inner.values()) and end <= total, (name, off, end, total)
    for (_, end, name), (off, _, nxt) in zip(spans, spans[1:]):
        assert end <= off, (name, nxt)
    assert spans[-1][1] == total == inner_bytes + sum(f(n, groups) for f in OWN.values())      # ... and end at bytes()
    assert plane_rows == groups + 1
    # what the layout admits for its inner calls (work_layout.h, the rule) is the offset of its first own region, and holds every layout an
    # inner call carves at the size it is called with -- INNER restates who is called with what from fourq_amd.hip: the grouped sum over n
    # rows and over 2 x groups, [s]G + [c]pk, DH_endo and MUL_endo over `groups` rows, the comb with its encoding over groups + 1
    assert inner_extent == spans[0][0] == own["d"]
    assert all(inner_extent >= f(n, groups) for f in INNER.values())
