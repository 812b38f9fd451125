"""The verifiable random function on the CPU (no GPU needed): the restatement (tests/vrf_ref.py) against the rows the real reference's point
functions produced (tests/golden/vrf.json), completeness, the soundness list, the statuses in their order of precedence, the torsion-shifted
Gamma, the keyed flavour, the header against the binding, and the work-buffer layout (vrf_layout.h) compiled with g++."""
import functools
import os
import re
import subprocess

import pytest

import adversarial_points
import keyset_ref
import ref_loader
import sig_ref
import vrf_ref as ref
from conftest import GOLDEN, ROOT, load_golden

N = ref.N
ALPHA_LENGTHS = {0, 1, 31, 32, 33, 95, 96, 97}


def rows():
    return load_golden("vrf.json", raw=True)["rows"]


def fields(r):
    return tuple(bytes.fromhex(r[k]) for k in ("dst", "sk", "pk", "alpha", "proof", "beta"))


@functools.lru_cache(maxsize=None)
def honest():
    """four honest rows of the fixture under one dst, with alpha of at least two bytes: pks, alphas, proofs, betas, dst"""
    dst = bytes.fromhex(rows()[0]["dst"])
    pick = [fields(r) for r in rows() if r["kind"] == "honest" and bytes.fromhex(r["dst"]) == dst and len(r["alpha"]) >= 4][:4]
    assert len(pick) == 4
    return [p[2] for p in pick], [p[3] for p in pick], [p[4] for p in pick], [p[5] for p in pick], dst


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vrf", os.path.join(GOLDEN, "make_vrf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "vrf.json")) as fh:
        assert mod.generate() == fh.read()


def test_fixture_covers_the_cases_it_promises():
    rs = rows()
    assert os.path.getsize(os.path.join(GOLDEN, "vrf.json")) < 64 * 1024
    assert len(rs) >= 20
    for ln in (1, 255):
        under = [r for r in rs if len(r["dst"]) // 2 == ln]
        assert {len(r["alpha"]) // 2 for r in under if r["kind"] == "honest"} == ALPHA_LENGTHS
        assert {r["kind"] for r in under if r["kind"] != "honest"} == {"gamma shifted by a point of order %d" % k for k in (7, 14)}
    # the end of pk32 || alpha || I2OSP(128, 2) || 0 || DST_prime behind Z_pad: L bytes take ceil((L + 17) / 128) more blocks
    blocks = lambda total: (total + 17 + 127) // 128
    assert sorted({blocks(32 + al + 3 + 1 + 1) for al in ALPHA_LENGTHS}) == [1, 2] and sorted({blocks(32 + al + 3 + 255 + 1) for al in ALPHA_LENGTHS}) == [3, 4]
    for r in rs:
        assert len(r["proof"]) == 192 and len(r["beta"]) == 128 and len(r["pk"]) == len(r["sk"]) == len(r["h32"]) == 64


def test_restatement_reproduces_the_golden_rows():
    for r in rows():
        dst, sk, pk, alpha, proof, beta = fields(r)
        assert sig_ref.keygen(sk) == pk
        assert ref.enc(ref.hash_point(pk, alpha, dst)).hex() == r["h32"]
        if r["kind"] == "honest":
            assert ref.prove(sk, pk, alpha, dst) == proof, r["kind"]
        else:
            assert ref.prove(sk, pk, alpha, dst).hex() == r["honest_proof"]
        assert ref.verify(pk, alpha, proof, dst) == (1, 0, beta)
        assert ref.proof_to_hash(proof, dst) == (beta, 0)
        assert ref.cleared(proof[:32])[1].hex() == r["w32"]


def test_a_gamma_shifted_by_torsion_is_accepted_with_the_honest_beta():
    """What hashing W instead of Gamma buys: a prover who adds a point of order 7 or 14 to Gamma and hashes the challenge again is accepted
    -- the verifier clears the cofactor before any ladder sees Gamma -- and beta does not move."""
    torsion = {}
    for label, T in adversarial_points.torsion():
        if label.startswith("seeded torsion"):
            torsion.setdefault(adversarial_points.order_in_392(T), T)                   # the first of each order, as the generator takes them
    shifted = [r for r in rows() if r["kind"] != "honest"]
    assert len(shifted) == 4
    for r in shifted:
        dst, sk, pk, alpha, proof, beta = fields(r)
        order = int(r["kind"].split()[-1])
        assert ref.prove(sk, pk, alpha, dst, shift=torsion[order]) == proof
        honest_proof = bytes.fromhex(r["honest_proof"])
        assert honest_proof[:32] != proof[:32]
        assert ref.verify(pk, alpha, honest_proof, dst) == (1, 0, beta) == ref.verify(pk, alpha, proof, dst)
        # ... while the honest c and s do not fit the shifted Gamma
        assert ref.verify(pk, alpha, proof[:32] + honest_proof[32:], dst) == (0, 0, ref.ZERO_BETA)


def test_soundness_every_tampering_fails_exactly_its_own_rows():
    pks, alphas, proofs, betas, dst = honest()
    labels = []
    for label, pk_t, a_t, p_t, dst_t, failing in ref.soundness_cases(pks, alphas, proofs, dst):
        for i in range(len(proofs)):
            got = ref.verify(pk_t[i], a_t[i], p_t[i], dst_t)
            assert got == ((0, 0, ref.ZERO_BETA) if i in failing else (1, 0, betas[i])), (label, i)
        labels.append(label)
    assert len(labels) == 8 and {"one flipped bit in " + w for w in ("gamma", "c", "s", "dst")} <= set(labels)


def test_inv392_is_the_inverse_of_the_cofactor():
    from fourq_amd import constants
    assert 392 * ref.INV392 % N == 1 and constants.INV392 == ref.INV392 and 0 < constants.INV392 < N
    text = open(os.path.join(ROOT, "fourq_amd", "csrc", "constants.inc")).read()
    words = re.search(r"SC_INV392\[4\] = \{ ([^}]*) \}", text).group(1).split(", ")
    assert sum(int(w.rstrip("ul"), 16) << (64 * i) for i, w in enumerate(words)) == ref.INV392


def test_statuses_in_their_order_of_precedence():
    pks, alphas, proofs, betas, dst = honest()
    pk, alpha, proof = pks[0], alphas[0], proofs[0]
    refused = lambda st: (0, st, ref.ZERO_BETA)
    not_on_curve, reserved = bytes([2] + [0] * 31), bytes([0] * 15 + [0x80] + [0] * 16)
    assert [sig_ref.decode_status(b)[0] for b in (reserved, not_on_curve, ref.NEUTRAL32)] == [16 + 1, 16 + 2, 16 + 3]
    c_is_n = proof[:32] + N.to_bytes(32, "little") + proof[64:]
    s_is_n = proof[:64] + N.to_bytes(32, "little")
    for bad in (reserved, not_on_curve, ref.NEUTRAL32):
        st = sig_ref.decode_status(bad)[0]
        assert ref.verify(bad, alpha, proof, dst) == refused(st)
        assert ref.verify(pk, alpha, bad + proof[32:], dst) == refused(st)
        assert ref.verify(bad, alpha, not_on_curve + proof[32:], dst) == refused(st)                 # the key before Gamma
        assert ref.verify(pk, alpha, bad + c_is_n[32:], dst) == refused(st)                          # decoding before the range
        assert ref.proof_to_hash(bad + proof[32:], dst) == (ref.ZERO_BETA, st)
    assert ref.verify(pk, alpha, c_is_n, dst) == refused(ref.SIG_S_RANGE) == ref.verify(pk, alpha, s_is_n, dst)
    assert ref.verify(pk, alpha, proof[:32] + (N - 1).to_bytes(32, "little") * 2, dst) == refused(0)
    assert ref.proof_to_hash(c_is_n, dst) == (betas[0], 0)                                          # c and s are not looked at


def test_a_pure_torsion_gamma_is_the_neutral_w():
    pks, alphas, proofs, _, dst = honest()
    seen = set()
    for label, T in adversarial_points.torsion():
        if not label.startswith("seeded torsion"):
            continue
        g32 = adversarial_points.encode(T)
        assert sig_ref.decode_status(g32)[0] == 0
        seen.add(adversarial_points.order_in_392(T))
        assert ref.verify(pks[0], alphas[0], g32 + proofs[0][32:], dst) == (0, ref.GAMMA_NEUTRAL, ref.ZERO_BETA), label
        assert ref.proof_to_hash(g32 + proofs[0][32:], dst) == (ref.ZERO_BETA, ref.GAMMA_NEUTRAL)
        # the range of c and s comes first
        assert ref.verify(pks[0], alphas[0], g32 + N.to_bytes(32, "little") + proofs[0][64:], dst)[1] == ref.SIG_S_RANGE
    assert {7, 14, 28, 56} <= seen and ref.GAMMA_NEUTRAL == 128


def test_keyed_verify_orders_the_key_set_first_and_equals_the_unkeyed_call():
    pks, alphas, proofs, betas, dst = honest()
    A = sig_ref.decode_status(pks[1])[1]
    order_2n = adversarial_points.encode((tuple((-c) % ref.o.P127 for c in A[0]), tuple((-c) % ref.o.P127 for c in A[1])))
    keys = [pks[0], order_2n, bytes([2] + [0] * 31), pks[2]]
    assert [keyset_ref.key_status(k) for k in keys] == [0, ref.KEYSET_NOT_ORDER_N, 16 + 2, 0]
    assert ref.verify_keyed(keys, 0, alphas[0], proofs[0], dst) == (1, 0, betas[0]) == ref.verify(pks[0], alphas[0], proofs[0], dst)
    assert ref.verify_keyed(keys, 3, alphas[2], proofs[2], dst) == (1, 0, betas[2])
    assert ref.verify_keyed(keys, 3, alphas[0], proofs[0], dst) == (0, 0, ref.ZERO_BETA)
    bad = bytes([2] + [0] * 31) + N.to_bytes(32, "little") * 2
    assert ref.verify_keyed(keys, 1, alphas[1], bad, dst) == (0, ref.KEYSET_NOT_ORDER_N, ref.ZERO_BETA)
    assert ref.verify_keyed(keys, 2, alphas[1], bad, dst) == (0, 16 + 2, ref.ZERO_BETA)
    assert ref.verify_keyed(keys, 4, alphas[1], bad, dst) == (0, ref.KEYSET_ID_RANGE, ref.ZERO_BETA)
    assert ref.verify_keyed(keys, 0, alphas[0], bad, dst) == (0, 16 + 2, ref.ZERO_BETA)


def test_header_and_binding_declare_the_same_new_symbols():
    from fourq_amd import _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_vrf_\w+)\s*\(([^;{]*)\)\s*;", header))
    arity = {"fourq_vrf_prove": 12, "fourq_vrf_verify": 14, "fourq_vrf_verify_keyed": 14, "fourq_vrf_proof_to_hash": 7}
    new = set(arity) | {n + "_dev" for n in arity} | {"fourq_vrf_reserve"}
    assert set(decls) == new == {n for n in _lib.PROTOTYPES if "vrf" in n}
    for name, args in decls.items():
        count = len([a for a in args.split(",") if a.strip()])
        assert count == len(_lib.PROTOTYPES[name][1]) == (2 if name == "fourq_vrf_reserve" else arity[name.replace("_dev", "")]), name
        assert _lib.PROTOTYPES[name][1] == _lib.PROTOTYPES[name.replace("_dev", "")][1], name
    assert re.search(r"#define\s+FOURQ_VRF_GAMMA_NEUTRAL\s+128\b", header) and _lib.VRF_GAMMA_NEUTRAL == 128 == ref.GAMMA_NEUTRAL
    codes = [int(v) for v in re.findall(r"#define\s+FOURQ_(?:SIG_S_RANGE|SIG_MSG_CLAMPED|OPRF_BLIND_ZERO|DLEQ_NONCE_ZERO|KEYSET_NOT_ORDER_N|KEYSET_ID_RANGE|VRF_GAMMA_NEUTRAL)\s+(\d+)", header)]
    assert len(codes) == len(set(codes)) == 7                                            # 128 was unused
    assert "verifiable random function" in header_raw
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600      # functions were added, no struct changed
    from fourq_amd import Engine, MultiEngine
    calls = ("vrf_prove", "vrf_verify", "vrf_verify_keyed", "vrf_proof_to_hash")
    assert all(callable(getattr(Engine, m)) and callable(getattr(Engine, m + "_dev")) for m in calls) and callable(Engine.vrf_reserve)
    assert all(callable(getattr(MultiEngine, m)) for m in calls)
    from fourq_amd import build
    assert {"vrf.hip.h", "vrf_layout.h"} <= set(build.HEADERS)


def test_bytes_module_carries_a_known_answer_the_restatement_confirms():
    from fourq_amd import vrf
    assert all(callable(getattr(vrf, f)) for f in ("prove", "verify", "proof_to_hash", "prove_many", "verify_many", "proof_to_hash_many"))
    sk, alpha = bytes.fromhex(vrf.KAT_SK), bytes.fromhex(vrf.KAT_ALPHA)
    pk = sig_ref.keygen(sk)
    assert pk.hex() == vrf.KAT_PK
    proof = ref.prove(sk, pk, alpha, vrf.KAT_DST)
    assert proof.hex() == vrf.KAT_PROOF
    assert ref.verify(pk, alpha, proof, vrf.KAT_DST) == (1, 0, bytes.fromhex(vrf.KAT_BETA))


# ---- the work-buffer layout (vrf_layout.h), compiled with g++ ---------------------------------------------------------------------------
def a(n):
    return (n + 255) & ~255


# own region -> bytes, in the order the header carves them behind `inner`; `affine` lies ON u
OWN = {
    "u": lambda n: 64 * n, "pk32": lambda n: 32 * n, "h32": lambda n: 32 * n, "g32": lambda n: 32 * n, "u32": lambda n: 32 * n, "v32": lambda n: 32 * n,
    "sc_a": lambda n: 32 * n, "sc_b": lambda n: 32 * n, "pair_sc": lambda n: 64 * n, "pair_pt": lambda n: 64 * n,
    "st_a": a, "st_b": a, "st_u": a, "st_v": a, "st_pre": a,
}
# what each inner call's layout takes at the size it is called with, from work_layout.h's and keyset_layout.h's structs
DOUBLE_MUL = lambda n: 320 * n + 2 * a(n) + 96 * n + a(n)
INNER = {
    "mul_rows": lambda n: 384 * n + a(n),
    "double_mul": DOUBLE_MUL,
    "keyset": lambda n: DOUBLE_MUL(n) + 96 * n + 96 * n + 32 * n + a(n),
    "msm_pair": lambda n: 320 * 2 * n + a(2 * n) + 96 * n + a(n) + 96 * (n // 2) + a(n // 2),
}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vrf_layout") / "vrf_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "vrf_layout_dump.cpp"), "-o", exe], check=True)

    def run(n):
        out = subprocess.run([exe, str(n)], check=True, capture_output=True, text=True).stdout
        return {name: int(value) for name, value in (line.split() for line in out.splitlines())}
    return run


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4095, 65537, 0xffffff00 // 2])
def test_vrf_regions_are_aligned_disjoint_behind_the_inner_layouts_and_end_at_the_total(layout, n):
    offs = layout(n)
    total, inner_bytes, planes, inner_extent = offs.pop("bytes"), offs.pop("inner_bytes"), offs.pop("planes"), offs.pop("inner_extent")
    inner = {k.split(".")[1]: v for k, v in offs.items() if k.startswith("inner.")}
    own = {k.split(".")[1]: v for k, v in offs.items() if k.startswith("own.")}
    assert own.pop("inner") == 0
    assert own.pop("affine") == own["u"]                                                # the comb's affine rows: u is dead by then, and as large
    assert inner == {name: f(n) for name, f in INNER.items()}
    assert inner_bytes == max(inner.values())
    assert list(own) == list(OWN)
    spans = [(off, off + OWN[name](n), name) for name, off in own.items()]
    assert spans == sorted(spans)                                                       # carved in the order the header lists them
    assert spans[0][0] == inner_bytes                                                   # the own regions start behind the largest inner layout ...
    for off, end, name in spans:
        assert off % 16 == 0 and off >= max(inner.values()) and end <= total, (name, off, end, total)
    for (_, end, name), (off, _, nxt) in zip(spans, spans[1:]):
        assert end <= off, (name, nxt)
    assert spans[-1][1] == total == inner_bytes + sum(f(n) for f in OWN.values())      # ... and end at bytes(), what fourq_vrf_reserve sizes
    assert planes == 1
    # what the layout admits for its inner calls (work_layout.h, the rule) is the offset of its first own region, and holds every layout an
    # inner call carves at the size it is called with -- INNER restates who is called with what from fourq_amd.hip: MUL_endo on encodings,
    # [s]G + [c]Y and its keyed sibling over n rows, the grouped sum over 2 n
    assert inner_extent == spans[0][0] == own["u"]
    assert all(inner_extent >= f(n) for f in INNER.values())
