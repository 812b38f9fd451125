"""Pins what the GPU tests of the grouped multi-scalar multiplication expect, before any GPU runs (no GPU needed).

tests/golden/msm.json holds the real reference's R1toAffine(MUL_endo(k_0, P_0) + MUL_endo(k_1, P_1) + ...) for thirteen groups of 1, 2, 3,
5 and 8 elements (tests/golden/make_msm.py).  Two other sources must give the same points: the Python oracle's ADD chained over the C
oracle's MUL_endo, and -- every P being [t]G -- the group law sum [k_i][t_i]G = [(sum k_i t_i) mod N]G through the C oracle, the identity
tests/test_gpu_msm.py builds its large shapes on.  The rest checks what needs no device: the four symbols in header and binding, the ABI
version, and the work-buffer layout compiled with g++."""
import os
import re
import subprocess

import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
import ref_loader
from conftest import GOLDEN, ROOT
from fourq_amd import codec

G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
NEUTRAL = ((0, 0), (1, 0))
NEUTRAL_ENC = bytes([1] + [0] * 31)
TOP = (1 << 256) - 1


def lift(points):
    """(n, 20) R1 rows of affine points: AffineToR1, as the C oracle's mul takes them"""
    P = codec.pack_points(points, 2)
    rows = np.zeros((len(points), 20), dtype=np.uint64)
    rows[:, 0:8] = P
    rows[:, 8] = 1
    rows[:, 12:20] = P
    return rows


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_msm", os.path.join(GOLDEN, "make_msm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "msm.json")) as fh:
        assert mod.generate() == fh.read()


def test_fixture_covers_the_cases_it_promises(golden):
    groups = golden("msm.json")["groups"]
    assert os.path.getsize(os.path.join(GOLDEN, "msm.json")) < 64 * 1024
    assert len(groups) >= 12 and {g["group_size"] for g in groups} == {1, 2, 3, 5, 8}
    assert all(len(g["k"]) == len(g["t"]) == len(g["P"]) == len(g["P_enc"]) == g["group_size"] for g in groups)
    assert {0, 1, o.N, TOP} <= {k for g in groups for k in g["k"]}
    neg = lambda P: (o.f2_neg(P[0]), P[1])
    assert any(g["group_size"] == 2 and g["k"][0] == g["k"][1] and g["P"][1] == neg(g["P"][0]) and g["R"] == NEUTRAL for g in groups)
    assert any(g["group_size"] == 2 and g["k"][0] == g["k"][1] and g["P"][0] == g["P"][1] and g["R"] != NEUTRAL for g in groups)
    assert any(g["group_size"] > 1 and not any(g["k"]) and g["R"] == NEUTRAL for g in groups)
    for g in groups:
        assert all(o.PointOnCurve(P) for P in g["P"]), g["_label"]
        assert [bytes(o.encode(*P)).hex() for P in g["P"]] == ["%064x" % e for e in g["P_enc"]], g["_label"]
        assert [o.decode(bytes.fromhex("%064x" % e)) for e in g["P_enc"]] == list(g["P"]), g["_label"]
        assert bytes(o.encode(*g["R"])).hex() == "%064x" % g["R_enc"], g["_label"]
        if g["R"] == NEUTRAL:
            assert bytes.fromhex("%064x" % g["R_enc"]) == NEUTRAL_ENC


def test_add_chain_over_the_c_oracle_gives_the_fixture(golden):
    for g in golden("msm.json")["groups"]:
        products = codec.unpack_points(oc.mul(oc.ENDO, codec.pack_scalars(list(g["k"])), lift(list(g["P"]))))
        acc = products[0]
        for B in products[1:]:
            acc = o.ADD(acc, o.R1toR2(B))
        assert o.R1toAffine(acc) == g["R"], g["_label"]
        # ... and in the opposite order: the canonical point does not depend on the order of folding
        acc = products[-1]
        for B in reversed(products[:-1]):
            acc = o.ADD(acc, o.R1toR2(B))
        assert o.R1toAffine(acc) == g["R"], g["_label"]


def test_group_law_through_the_c_oracle_gives_the_fixture(golden):
    groups = golden("msm.json")["groups"]
    table = oc.table(oc.ENDO, G1_WORDS)
    # the points are what the fixture says they are: P = [t]G
    ts = [t for g in groups for t in g["t"]]
    assert codec.unpack_points(oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(ts), None, table))) == [P for g in groups for P in g["P"]]
    sums = [sum(k * t for k, t in zip(g["k"], g["t"])) % o.N for g in groups]
    want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, table))
    assert codec.unpack_points(want) == [g["R"] for g in groups]
    assert [bytes(r).hex() for r in oc.encode(want)] == ["%064x" % g["R_enc"] for g in groups]


def test_header_and_binding_declare_the_same_new_symbols():
    from fourq_amd import _lib
    header_raw = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_raw, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(fourq_msm_\w+)\s*\(([^;{]*)\)\s*;", header))
    new = {"fourq_msm_affine_batch", "fourq_msm_bytes_batch"}
    new |= {n + "_dev" for n in new}
    assert set(decls) == new == {n for n in _lib.PROTOTYPES if "msm" in n}
    for name, args in decls.items():
        arity = len([a for a in args.split(",") if a.strip()])
        assert arity == len(_lib.PROTOTYPES[name][1]) == (7 if "bytes" in name else 6), name
        assert re.search(r"size_t\s+groups\s*,\s*size_t\s+group_size\s*$", args), name
    assert "#define FOURQ_ABI_VERSION 600" in header_raw and _lib.ABI_VERSION == 600
    from fourq_amd import Engine
    assert all(callable(getattr(Engine, m)) for m in ("msm", "msm_bytes", "msm_dev", "msm_bytes_dev"))


def test_groups_must_divide_the_batch():
    from fourq_amd import Engine
    assert Engine._groups(12, 3) == (4, 3) and Engine._groups(0, 5) == (0, 5)
    for n, size in ((7, 2), (1, 3), (4, 0), (4, -1)):
        with pytest.raises(ValueError):
            Engine._groups(n, size)


# ---- the work buffer ------------------------------------------------------------------------------------------------------------------
def a(n):
    return (n + 255) // 256 * 256


# bytes each region's users read or write for n elements: the ladder's rows, one decode code per element, and partial sums of 12 words with
# one code each -- at most n / 2 after the first fold pass and n / 4 after the second (a pass leaves ceil(m / 64) <= m / 2 rows of m >= 2)
NEED = {"rows_in": lambda n: n * 160, "rows_out": lambda n: n * 160, "st_decode": lambda n: n, "part_a": lambda n: n // 2 * 96, "st_a": lambda n: n // 2,
        "part_b": lambda n: n // 4 * 96, "st_b": lambda n: n // 4}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_layout") / "msm_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "msm_layout_dump.cpp"), "-o", exe], check=True)

    def run(n):
        return {name: int(value) for name, value in (line.split() for line in subprocess.run([exe, str(n)], check=True, capture_output=True, text=True).stdout.splitlines())}
    return run


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 1023, 4095, 4097, 65536, 65537, 0xffffff00])
def test_msm_regions_are_aligned_disjoint_and_end_at_the_total(layout, n):
    offs = layout(n)
    total, sig_verify = offs.pop("bytes"), offs.pop("sig_verify_bytes")
    assert set(offs) == set(NEED)
    spans = sorted((off, off + NEED[name](n), name) for name, off in offs.items())
    assert spans[0][0] == 0
    for off, end, name in spans:
        assert off % 16 == 0 and end <= total, (name, off, end, total)
    for (_, end, name), (off, _, nxt) in zip(spans, spans[1:]):
        assert end <= off, (name, nxt)
    assert [name for _, _, name in spans if NEED[name](n)] == [name for name in NEED if NEED[name](n)]     # carved in the order the header lists them
    assert total == 2 * n * 160 + a(n) + n // 2 * 96 + a(n // 2) + n // 4 * 96 + a(n // 4)
    assert offs["st_b"] + a(n // 4) == total
    # fourq_ctx_reserve takes the maximum over the layouts: this one stays below the signature check's, so reserve does not grow
    assert total <= sig_verify == 2 * n * 160 + 3 * a(n) + 3 * n * 32


@pytest.mark.parametrize("group_size", [2, 3, 5, 63, 64, 65, 127, 129, 4096, 4097, 262144, 262145])
def test_partial_regions_hold_every_pass(group_size):
    """The fold factor is 64: pass 1 writes part_a, pass 2 part_b, pass 3 part_a again, pass 4 part_b.  Rows left after each pass, for any number of groups,
    against the rows the regions hold."""
    for groups in (1, 3, 67):
        n, m, room = groups * group_size, group_size, [groups * group_size // 2, groups * group_size // 4]
        passes = 0
        while m > 1:
            m = -(-m // 64)
            assert groups * m <= room[passes % 2], (groups, group_size, passes)
            passes += 1
        assert passes == (1 if group_size <= 64 else 2 if group_size <= 4096 else 3 if group_size <= 262144 else 4)
        assert n // 2 * 96 == NEED["part_a"](n)
