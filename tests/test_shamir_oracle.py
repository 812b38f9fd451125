"""Threshold sharing on the CPU (no GPU needed): the restatement (tests/shamir_ref.py) against the rows the real reference's point functions
produced (tests/golden/shamir.json), the algebra (the coefficients sum to 1, every t-subset reconstructs), the Horner step's quotient estimate
at its bounds, the header against the binding, and the work-buffer layout (shamir_layout.h) compiled with g++."""
import itertools
import os
import random
import re
import subprocess

import pytest

import ref_loader
import shamir_ref as ref
from conftest import GOLDEN, ROOT, load_golden

N = ref.N
TOP = (1 << 256) - 1


def fixture():
    return load_golden("shamir.json", raw=True)


def ints(hexes):
    return [int(h, 16) for h in hexes]


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_shamir", os.path.join(GOLDEN, "make_shamir.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "shamir.json")) as fh:
        assert mod.generate() == fh.read()


def test_fixture_covers_the_cases_it_promises():
    fx = fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "shamir.json")) < 64 * 1024
    assert fx["ids"] == [1, 2, 7, (1 << 32) - 1]
    assert sorted({p["t"] for p in fx["polys"]}) == [1, 2, 3, 5]
    coeffs = {a for p in fx["polys"] for a in ints(p["coeffs"])}
    assert {1, N - 1, N + 1, TOP} <= coeffs and any(a > N for a in coeffs - {N + 1, TOP})
    assert len(fx["sets"]) == 3 and all({1, (1 << 32) - 1} <= set(s["ids"]) for s in fx["sets"][1:])
    assert len(fx["exponent"]["ids"]) == 3


def test_restatement_reproduces_the_golden_rows():
    fx = fixture()
    ids = fx["ids"]
    for p in fx["polys"]:
        poly = ints(p["coeffs"])
        blocks, status = ref.shares([poly], ids)
        assert [b[0] for b in blocks] == ints(p["shares"]) and status == [0] * len(ids)
        commits = ref.commitments(poly)
        assert [c.hex() for c in commits] == p["commits"]
        for x, share, public in zip(ids, ints(p["shares"]), p["public"]):
            assert ref.public_share(commits, x) == (bytes.fromhex(public), 0)
            assert ref.verify(commits, x, share) == (1, 0)
            assert ref.verify(commits, x, share ^ 1) == (0, 0)
    for s in fx["sets"]:
        assert ref.lagrange(s["ids"]) == (ints(s["lambda"]), 0)
    e = fx["exponent"]
    out, status = ref.combine_points(e["ids"], [[bytes.fromhex(p)] for p in e["points"]])
    assert out == [bytes.fromhex(e["combined"])] and status == [0]


def test_statuses_of_the_restatement():
    assert ref.lagrange([3, 0, 3]) == ([0, 0, 0], ref.ID_ZERO)                          # the id 0 comes first
    assert ref.lagrange([3, 5, 3]) == ([0, 0, 0], ref.ID_REPEATED)
    assert ref.lagrange([9]) == ([1], 0)
    assert ref.shares([[5, 6]], [0, 1]) == ([[0], [11]], [ref.ID_ZERO, 0])
    commits = ref.commitments([5, 6, 7])
    assert ref.public_share(commits, 0) == (ref.ZERO32, ref.ID_ZERO)
    assert ref.verify(commits, 2, ref.horner([5, 6, 7], 2) + N) == (0, ref.SIG_S_RANGE)
    assert ref.commitments([N, 1])[0] == ref.NEUTRAL32
    assert ref.public_share(ref.commitments([N, 1]), 2) == (ref.ZERO32, ref.REFUSED_NEUTRAL)
    assert ref.combine_points([1, 1], [[commits[0]], [commits[1]]]) == ([ref.ZERO32], [ref.ID_REPEATED])
    # a polynomial that vanishes at 7: both sides of the check are the neutral point, which compares equal
    a1, a2 = 11, 13
    vanishing = [-(7 * a1 + 49 * a2) % N, a1, a2]
    assert ref.horner(vanishing, 7) == 0 and ref.verify(ref.commitments(vanishing), 7, 0) == (1, 0)
    assert ref.public_share(ref.commitments(vanishing), 7) == (ref.NEUTRAL32, 0)


def test_the_coefficients_sum_to_one_and_every_t_subset_reconstructs():
    rng = random.Random(77)
    five = [1, 2, 7, 1000003, (1 << 32) - 1]
    for t in (1, 2, 3, 5):
        poly = [rng.randrange(1 << 256) for _ in range(t)]
        blocks, _ = ref.shares([poly], five)
        for pick in itertools.combinations(range(5), t):
            ids = [five[i] for i in pick]
            lam, st = ref.lagrange(ids)
            assert st == 0 and sum(lam) % N == 1
            assert ref.combine(ids, [blocks[i] for i in pick]) == ([poly[0] % N], 0)
    # one share too few says nothing: another polynomial through the same t - 1 points has another secret
    poly = [rng.randrange(N) for _ in range(3)]
    blocks, _ = ref.shares([poly], five)
    assert ref.combine(five[:2], blocks[:2])[0] != [poly[0]]


def test_horner_step_quotient_estimate_at_its_bounds():
    """shamir.hip.h's sc_horner_step: the quotient from the top words is never above floor(v / N) and at most 2 below, so two conditional
    subtractions give the canonical residue -- at the largest accumulator, id and coefficient, and on random operands"""
    mu = (1 << 512) // N
    assert mu.bit_length() == 267
    rng = random.Random(78)
    accs = [0, 1, N - 1, N - 2, 1 << 245] + [rng.randrange(N) for _ in range(300)]
    xs = [0, 1, 2, (1 << 32) - 1, 1 << 31] + [rng.randrange(1 << 32) for _ in range(20)]
    coeffs = [0, 1, N - 1, N, N + 1, TOP, 1 << 255] + [rng.randrange(1 << 256) for _ in range(20)]
    worst = 0
    for acc in accs:
        for x in xs:
            for a in coeffs:
                r, q, v = ref.horner_step_words(acc, x, a, mu)
                assert v < 1 << 279 and q < 1 << 35 and 0 <= v // N - q <= 2 and v - q * N < 1 << 248
                assert r == (acc * x + a) % N
                worst = max(worst, v // N - q)
    assert worst >= 1                                                                    # the second subtraction is not dead code


def test_header_and_binding_declare_the_same_new_symbols():
    from fourq_amd import _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_shamir_\w+)\s*\(([^;{]*)\)\s*;", header))
    arity = {"fourq_shamir_shares": 8, "fourq_shamir_lagrange": 6, "fourq_shamir_combine": 7, "fourq_shamir_combine_points": 7, "fourq_shamir_public_shares": 7,
             "fourq_shamir_verify": 9}
    new = set(arity) | {n + "_dev" for n in arity} | {"fourq_shamir_reserve"}
    assert set(decls) == new == {n for n in _lib.PROTOTYPES if "shamir" in n}
    for name, args in decls.items():
        count = len([a for a in args.split(",") if a.strip()])
        assert count == len(_lib.PROTOTYPES[name][1]) == (3 if name == "fourq_shamir_reserve" else arity[name.replace("_dev", "")]), name
        assert _lib.PROTOTYPES[name][1] == _lib.PROTOTYPES[name.replace("_dev", "")][1], name
    for name in new:
        assert not name.endswith(("_batch", "_batch_dev")) and "hash_to" not in name and "map_to" not in name
    assert re.search(r"#define\s+FOURQ_SHAMIR_ID_ZERO\s+144\b", header) and _lib.SHAMIR_ID_ZERO == 144 == ref.ID_ZERO
    assert re.search(r"#define\s+FOURQ_SHAMIR_ID_REPEATED\s+160\b", header) and _lib.SHAMIR_ID_REPEATED == 160 == ref.ID_REPEATED
    assert re.search(r"#define\s+FOURQ_SHAMIR_MAX_T\s+4096\b", header) and _lib.SHAMIR_MAX_T == 4096 == ref.MAX_T
    codes = [int(v) for v in re.findall(r"#define\s+FOURQ_(?:SIG_S_RANGE|SIG_MSG_CLAMPED|OPRF_BLIND_ZERO|DLEQ_NONCE_ZERO|KEYSET_NOT_ORDER_N|KEYSET_ID_RANGE|VRF_GAMMA_NEUTRAL|"
                                             r"SHAMIR_ID_ZERO|SHAMIR_ID_REPEATED)\s+(\d+)", header)]
    assert len(codes) == len(set(codes)) == 9 and all(c % 16 == 0 for c in codes)       # above every 16 + FOURQ_DECODE_*
    assert "threshold sharing" in header_raw
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600      # functions were added, no struct changed
    from fourq_amd import Engine
    calls = ("shamir_shares", "shamir_lagrange", "shamir_combine", "shamir_combine_points", "shamir_public_shares", "shamir_verify")
    assert all(callable(getattr(Engine, m)) and callable(getattr(Engine, m + "_dev")) for m in calls)
    assert callable(Engine.shamir_reserve) and callable(Engine.shamir_commitments)
    from fourq_amd import build, shamir
    assert {"shamir.hip.h", "shamir_layout.h"} <= set(build.HEADERS)
    assert all(callable(getattr(shamir, f)) for f in ("split", "shares_of", "commitments", "public_share", "verify_share", "lagrange", "combine", "combine_points",
                                                      "combine_points_many"))


# ---- the work-buffer layout (shamir_layout.h), compiled with g++ -------------------------------------------------------------------------
def a(n):
    return (n + 255) & ~255


# own region -> bytes, in the order the header carves them behind `inner`
OWN = {
    "sc": lambda rows, t: 32 * rows * t, "pt": lambda rows, t: 32 * rows * t, "lambda": lambda rows, t: 32 * t,
    "pub32": lambda rows, t: 32 * rows, "g32": lambda rows, t: 32 * rows, "affine": lambda rows, t: 64 * rows,
    "flags": lambda rows, t: a(rows * t), "st_set": lambda rows, t: 256, "st_pub": lambda rows, t: a(rows), "st_comb": lambda rows, t: a(rows),
}
# what each inner call's layout takes at the size it is called with, from work_layout.h's structs: the grouped sum over rows x t elements
# (Msm), the comb with its encoding over `rows` scalars (Sig)
MSM = lambda n: 320 * n + a(n) + 96 * (n // 2) + a(n // 2) + 96 * (n // 4) + a(n // 4)
INNER = {"msm_rows": lambda rows, t: MSM(rows * t), "comb_encode": lambda rows, t: 160 * rows + a(rows)}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shamir_layout") / "shamir_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "shamir_layout_dump.cpp"), "-o", exe], check=True)

    def run(rows, t):
        out = subprocess.run([exe, str(rows), str(t)], check=True, capture_output=True, text=True).stdout
        return {name: int(value) for name, value in (line.split() for line in out.splitlines())}
    return run


@pytest.mark.parametrize("rows,t", [(1, 1), (1, 4096), (3, 5), (255, 1), (256, 3), (257, 3), (65536, 3), (1024, 256), (0xffffff00 // 4096, 4096), (0xffffff00, 1)])
def test_shamir_regions_are_aligned_disjoint_behind_the_inner_layouts_and_end_at_the_total(layout, rows, t):
    offs = layout(rows, t)
    total, inner_bytes, planes, plane_rows, inner_extent = (offs.pop(k) for k in ("bytes", "inner_bytes", "planes", "plane_rows", "inner_extent"))
    inner = {k.split(".")[1]: v for k, v in offs.items() if k.startswith("inner.")}
    own = {k.split(".")[1]: v for k, v in offs.items() if k.startswith("own.")}
    assert own.pop("inner") == 0
    assert inner == {name: f(rows, t) for name, f in INNER.items()}
    assert inner_bytes == max(inner.values()) >= MSM(rows * t)                         # `inner` covers Msm::bytes(rows * t)
    assert list(own) == list(OWN)
    spans = [(off, off + OWN[name](rows, t), name) for name, off in own.items()]
    assert spans == sorted(spans)                                                       # carved in the order the header lists them
    assert spans[0][0] == inner_bytes                                                   # the own regions start behind the largest inner layout ...
    for off, end, name in spans:
        assert off % 16 == 0 and off >= inner_bytes and end <= total, (name, off, end, total)
    for (_, end, name), (off, _, nxt) in zip(spans, spans[1:]):
        assert end <= off, (name, nxt)
    assert spans[-1][1] == total == inner_bytes + sum(f(rows, t) for f in OWN.values())      # ... and end at bytes(), what fourq_shamir_reserve sizes
    assert planes == 1 and plane_rows == rows                                           # the comb's rows
    assert inner_extent == spans[0][0] == own["sc"]
    assert all(inner_extent >= f(rows, t) for f in INNER.values())
