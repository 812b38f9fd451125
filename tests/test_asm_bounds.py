"""Limb bounds of the GENERATED gfx950 bodies (fourq_amd/csrc/ladder_asm_gfx950.inc), on the CPU: tools/asmgen/bounds.py runs every body's
instruction stream on intervals under the contract table (bounds.CONTRACTS, the operand types of the call sites) and proves that no
multiply-add operand, accumulator or carry shift leaves its range; bounds.CHAINS proves that every output fits wherever it goes next.
fp127.hip.h's static_asserts cover the C++ formulas; this covers the instruction streams that run in their place.

The analysis must bite (wider inputs, mutated bodies and a negative input to an unsigned body are reported), it must be sound (every
value sim.run computes lies in the interval the analysis gave that instruction), and at the corners of every contract -- limbs at their
extremes, sign patterns that maximise the first products' columns, top limbs in [2^23, 2^24) -- the bodies must still compute the oracle's
residues, with outputs inside the proven intervals."""
import os
import random
import re
import sys
import time
import zlib

import pytest

import curve4q_oracle as o
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools", "asmgen"))
import bounds as bd                # noqa: E402
import sim                         # noqa: E402

P = (1 << 127) - 1
M32 = (1 << 32) - 1
BODIES = ("DBL", "DBLT", "ADD", "STEP", "TAU", "UPSILON", "CHI", "TAUDUAL", "R1TOR2", "TABLEADD")


def _products():
    """the MULU / SQRU instances the corner tests run: the bound-1 product and the extremes of what the static_asserts admit"""
    mu = bd.mulu_admitted()
    pick = {(1, 1), max(mu), max(mu, key=lambda ab: ab[1]), max(mu, key=lambda ab: (2 * ab[0] + 1) * ab[1])}
    return ["MULU<%d,%d>" % ab for ab in sorted(pick)] + ["SQRU<%d>" % a for a in bd.sqru_admitted()]


CORNER_CONTRACTS = list(BODIES) + _products()


@pytest.fixture(scope="module")
def proven():
    t0 = time.time()
    outs, margins = bd.prove_all()
    return outs, margins, time.time() - t0


def test_contract_table_covers_every_shipped_body():
    assert set(bd.shipped()) == set(BODIES) | {"MULU", "SQRU"}
    assert {bd.body_of(n) for n in bd.CONTRACTS} == set(bd.shipped())
    import test_asm_bodies as tab                                   # the same text the residue tests read
    assert {k: [t for _, t in v] for k, v in bd.shipped().items()} == tab.BODY_TEXT


def test_restated_header_bounds_match_fp127_and_the_wrappers():
    """bounds.py restates fp127.hip.h's UNIT, LIMB_MASK, bias_limb and cols_ok, and the static_asserts of fe2_mul_asm / fe2_sqr_asm that
    select the admitted (A, B): a change to any of them must show up here"""
    fp = open(os.path.join(ROOT, "fourq_amd", "csrc", "fp127.hip.h")).read()
    assert "constexpr u64 UNIT = (1ull << 26) + (1ull << 15);" in fp and bd.UNIT == (1 << 26) + (1 << 15)
    assert "constexpr u32 LIMB_BITS = 26;" in fp and "LIMB_MASK = (1u << LIMB_BITS) - 1;" in fp
    assert "return (u32)k * (i == 0 ? (LIMB_MASK - 7) : LIMB_MASK);" in fp
    assert "return weighted * 5 * 8 <= ((~0ull - (1ull << 41)) / (UNIT * UNIT));" in fp
    mul = fp[fp.index("FQ_DEV Fe2<1> fe2_mul_asm"):fp.index("FQ_DEV Fe2<1> fe2_sqr_asm")]      # the wrappers live beside the products they replace
    sqr = fp[fp.index("FQ_DEV Fe2<1> fe2_sqr_asm"):fp.index("// ---- the flavours of a GF(p^2) product")]
    assert re.findall(r"static_assert\((.*?), \"", mul) == ["cols_ok((u64)(2 * A + 1) * B)", "(u64)8 * B * UNIT < (1ull << 32)"]
    assert "fe_neg(a.im)" in mul
    assert re.findall(r"static_assert\((.*?), \"", sqr) == ["cols_ok((u64)(2 * A + 1) * (2 * A))", "(u64)8 * (2 * A) * UNIT < (1ull << 32)"]
    assert "fe_add(a.re, a.im)" in sqr and "fe_sub(a.re, a.im)" in sqr and "fe_dbl(a.re)" in sqr
    # the restated cols_ok agrees with the header's at its boundary
    lim = (M32 << 32 | M32) - (1 << 41)
    for w in range(1, 200):
        assert bd.cols_ok(w) == (w * 40 <= lim // (bd.UNIT * bd.UNIT))
    assert (1, 1) in bd.mulu_admitted() and (1, 7) in bd.mulu_admitted() and (1, 8) not in bd.mulu_admitted()
    assert bd.sqru_admitted() == [1, 2, 3]


def test_every_body_is_proven_and_every_chain_edge_closes(proven):
    outs, margins, took = proven
    print()
    print(bd.report(outs, margins))
    assert bd.check_chains(outs) == []
    # the contract the comments state: products come out of bound 1, limb 1 a little below zero at worst; table entries tight
    for name in ("DBL", "DBLT", "ADD", "STEP", "TAU", "UPSILON", "CHI", "TAUDUAL"):
        for op in ("X", "Y", "Z"):
            assert not bd.within(outs[name][op], bd.signed(1)), (name, op)
    for name, ops in (("R1TOR2", "NDEF"), ("TABLEADD", ("qN", "qD", "qE", "qF"))):
        for op in ops:
            assert all(0 <= lo and hi < bd.UNIT for lo, hi in outs[name][op]), (name, op)
    assert took < 20


def test_analysis_reports_xyz_widened_to_two_units():
    for name in ("DBLT", "STEP"):
        for neg in bd.neg_values(name):
            a = bd.analyse(name, neg, override={k: bd.signed(2) for k in ("X", "Y", "Z")})
            assert a.findings, name
            f = a.findings[0]
            assert "v_mad_i64_i32 operand" in f.what and f.text.startswith("v_mad_i64_i32"), f
            assert f.lineno in {n for n, _ in bd.shipped()[name]}


def _prefix_interval(name, lines, upto, reg):
    a = bd.Analysis(name, lines[:upto], bd.input_regs(name)).run()
    return a.regs[reg]


def test_analysis_reports_a_wrap_operand_shifted_by_four():
    """every `<< 3` of DBLT made `<< 4`, one at a time: reported exactly when sixteen times the operand's proven bound leaves a signed
    32-bit operand (which happens for the eightfold of E and F, never for the inputs of bound 1)"""
    lines = bd.shipped()["DBLT"]
    flagged = 0
    for k, (n, t) in enumerate(lines):
        m = re.fullmatch(r"(v_lshlrev_b32_e(?:32|64)) (v\d+), 3, (\S+)", t)
        if not m:
            continue
        mut = list(lines)
        mut[k] = (n, "%s %s, 4, %s" % m.groups())
        a = bd.analyse("DBLT", 0, lines=mut)
        src = _prefix_interval("DBLT", lines, k, m.group(3))
        overflows = bd.fit((src[0] * 16, src[1] * 16), *bd.I32) is None
        assert bool(a.findings) == overflows, (n, t, src)
        if overflows:
            flagged += 1
            assert "operand %s" % m.group(2) in a.findings[0].what and a.findings[0].lineno > n
    assert flagged >= 8


def test_analysis_reports_an_arithmetic_carry_shift_made_logical():
    for name in ("DBLT", "ADD", "TAU"):
        lines = bd.shipped()[name]
        k = next(i for i, (_, t) in enumerate(lines) if t.startswith("v_ashrrev_i64"))
        mut = list(lines)
        mut[k] = (lines[k][0], lines[k][1].replace("v_ashrrev_i64", "v_lshrrev_b64"))
        a = bd.analyse(name, 0, lines=mut)
        assert a.findings and a.findings[0].lineno == lines[k][0] and "v_lshrrev_b64 operand" in a.findings[0].what, name


def test_analysis_reports_negative_limbs_for_an_unsigned_body():
    a = bd.analyse("MULU<1,1>", 0, override={"B": bd.signed(1)})
    assert a.findings and "v_mad_u64_u32 operand %25" in a.findings[0].what
    a = bd.analyse("SQRU<1>", 0, override={"im": bd.signed(1)[:5]})
    assert a.findings and "v_mad_u64_u32 operand" in a.findings[0].what
    # tighten (R1TOR2) assumes |X + Y| <= 2 UNIT: X, Y of bound 3 can make its biased sum negative
    a = bd.analyse("R1TOR2", 0, override={"X": bd.signed(3), "Y": bd.signed(3)})
    assert any("v_lshrrev_b32 operand" in f.what for f in a.findings)


# ---- soundness and residues at the corners ----------------------------------------------------------------------------------------------
def _val(limbs):
    return sum(l << (26 * i) for i, l in enumerate(limbs)) % P


def _fe2(limbs):
    return (_val(limbs[:5]), _val(limbs[5:]))


def _s32(x):
    return x - (1 << 32) if x & (1 << 31) else x


def expected(name, v, neg):
    """the oracle's residues of a body's outputs for input residues v = {operand: (re, im)}"""
    body = bd.body_of(name)
    if body in ("DBL", "DBLT"):
        w = o.DBL((v["X"], v["Y"], v["Z"]))
        out = {"X": w[0], "Y": w[1], "Z": w[2]}
        if body == "DBLT":
            out["T"] = o.f2_mul(w[3], w[4])
        return out
    if body in ("ADD", "STEP"):
        e = (v["N"], v["D"], v["E"], v["F"])
        chosen = o.R2neg(e) if neg else e
        if body == "ADD":
            r = o.ADD_core((o.f2_add(v["X"], v["Y"]), o.f2_sub(v["Y"], v["X"]), v["Z"], v["T"]), chosen)
        else:
            r = o.ADD(o.DBL((v["X"], v["Y"], v["Z"])), chosen)
        return dict(zip(("X", "Y", "Z", "Ta", "Tb"), r))
    if body in ("TAU", "UPSILON", "CHI"):
        fn = {"TAU": o.tau, "UPSILON": o.upsilon, "CHI": o.chi}[body]
        return dict(zip("XYZ", fn((v["X"], v["Y"], v["Z"]))[:3]))
    if body == "TAUDUAL":
        V = o.tau_dual((v["X"], v["Y"], v["Z"]))
        V3 = o.R1toR3(V)
        return {"X": V[0], "Y": V[1], "Z": V[2], "N3": V3[0], "D3": V3[1], "F3": V3[3]}
    if body == "R1TOR2":
        return dict(zip("NDEF", o.R1toR2((v["X"], v["Y"], v["Z"], v["Ta"], v["Tb"]))))
    if body == "TABLEADD":
        r = o.R1toR2(o.ADD_core((v["N3"], v["D3"], v["E3"], v["F3"]), (v["qN"], v["qD"], v["qE"], v["qF"])))
        return dict(zip(("qN", "qD", "qE", "qF"), r))
    if body == "MULU":
        assert _val(v["na"]) == (-v["A"][1]) % P
        return {"C": o.f2_mul(v["A"], v["B"])}
    if body == "SQRU":
        return {"C": o.f2_sqr(v["a"])}
    raise KeyError(name)


def run_checked(name, vec, neg, analysis, outs):
    """sim.run of one input vector: every value written inside the analysed interval of that instruction; returns the output registers"""
    trace = analysis.trace
    pos = [0]

    def check(ln, regs):
        lineno, text, w32, w64 = trace[pos[0]]
        assert text == ln
        for r, iv in w32:
            if iv is not None:
                assert (regs[r] - iv[0]) % (1 << 32) <= iv[1] - iv[0], (name, lineno, ln, r, regs[r], iv)
        for op, iv in w64:
            lo, hi = bd.Analysis._pair(op)
            x = regs[lo] | regs[hi] << 32
            if analysis.signed and x >> 63:
                x -= 1 << 64
            assert iv is not None and iv[0] <= x <= iv[1], (name, lineno, ln, op, x, iv)
        pos[0] += 1
    regs = sim.run([t for _, t in bd.shipped()[bd.body_of(name)]], bd.registers(name, vec, neg), trace=check)
    assert pos[0] == len(trace)
    for op, ivs in outs[name].items():
        base = bd.operands(name)[op][0]
        for i, (lo, hi) in enumerate(ivs):
            assert (regs["%%%d" % (base + i)] - lo) % (1 << 32) <= hi - lo, (name, op, i)
    return regs


@pytest.mark.parametrize("name", CORNER_CONTRACTS)
def test_sound_and_oracle_residues_at_the_corners(name, proven):
    outs = proven[0]
    rng = random.Random(zlib.crc32(name.encode()))
    count = 40 if bd.body_of(name) in ("MULU", "SQRU") else 24
    vecs = bd.corner_vectors(name, rng, count)
    for neg in bd.neg_values(name):
        analysis = bd.analyse(name, neg)
        assert not analysis.findings
        for vec in vecs:
            regs = run_checked(name, vec, neg, analysis, outs)
            v = {k: (_fe2(l) if len(l) == 10 else l) for k, l in vec.items()}
            if bd.body_of(name) == "SQRU":
                v = {"a": _fe2([vec["t"][i] // 2 for i in range(5)] + vec["im"])}
            for op, res in expected(name, v, neg).items():
                base = bd.operands(name)[op][0]
                got = _fe2([_s32(regs["%%%d" % (base + i)]) for i in range(10)])
                assert got == res, (name, neg, op)


def test_random_points_are_sound(proven):
    """the ladder's own inputs (random curve points, canonical limbs) through the ladder bodies: inside the analysed intervals too"""
    outs = proven[0]
    rng = random.Random(2611)
    for name in ("DBLT", "ADD"):
        for neg in bd.neg_values(name):
            analysis = bd.analyse(name, neg)
            for _ in range(3):
                Q = o.MUL_endo(rng.getrandbits(200) | 1, o.AffineToR1(o.Gx, o.Gy))
                e = o.R1toR2(o.MUL_endo(rng.getrandbits(200) | 1, o.AffineToR1(o.Gx, o.Gy)))
                limbs = lambda x: [(x >> (26 * i)) & ((1 << 26) - 1) for i in range(5)]  # noqa: E731
                fe = lambda a: limbs(a[0]) + limbs(a[1])  # noqa: E731
                vec = {"X": fe(Q[0]), "Y": fe(Q[1]), "Z": fe(Q[2]), "T": fe(o.f2_mul(Q[3], Q[4]))}
                vec.update({k: fe(c) for k, c in zip("NDEF", e)})
                if name == "DBLT":
                    vec = {k: vec[k] for k in "XYZ"}
                run_checked(name, vec, neg, analysis, outs)
