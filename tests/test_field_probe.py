"""The probe of tests/test_gpu_field_corners.py (tests/hip/field_flavour_probe.hip) and its Python side (tests/field_model.py), on the CPU:

* the probe compiles through fourq_amd/build.py's compile_unit and its kernels own every register the Gen entries clobber;
* every instantiation the library's four translation units make of the probed families has an id in FQ_PROBE_TABLE (listed from the
  units' LLVM IR, where the linkage names of inlined template instances survive), and so has the frontier of every product's
  static_asserts -- with both sides of wrap_operands_signed's split and of pmul's operand swap;
* field_model.py's restatement of those static_asserts agrees with the headers' text;
* the model -- the headers' column loops on Python integers, every 32-bit operand and 64-bit accumulator range-checked -- meets on
  every vector of every entry the two conditions the GPU test demands (residue and bound), and overflows where the asserts refuse."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT
import field_model as fm

CSRC = os.path.join(ROOT, "fourq_amd", "csrc")
TABLE = fm.probe_table()


def build_field_probe(out_dir, chain=False):
    """chain: as an FQ_CHAIN=1 unit, where add_table's and dbl()'s MUL_GROUP products are the chained ones"""
    from test_asm_probe import build_probe
    return build_probe(out_dir, fm.PROBE_SRC, "field_flavour_probe" + ("_chain" if chain else ""), ["-DFQ_CHAIN=1"] if chain else [])


def test_probe_owns_the_gen_entries_registers_and_builds(tmp_path):
    from fourq_amd import build as fb
    listing = str(tmp_path / "field_flavour_probe.s")
    flags = [f for f in fb.HIPCC_FLAGS if not f.startswith("-Rpass")] + ["-I" + fb.SRC_DIR]
    subprocess.run([fb._hipcc()] + flags + ["--cuda-device-only", "-S", "-o", listing, fm.PROBE_SRC], check=True, capture_output=True)
    fb.check_register_ranges(listing)                             # raises RegisterOwnershipError if a kernel does not own what it names
    text = open(listing).read()
    assert re.search(r"\bv255\b", text)                           # the generated products' temporaries are in the Gen kernels
    alloc = [int(x) for x in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    assert len(alloc) == len(TABLE), (len(alloc), len(TABLE))     # one kernel per id
    gen = sum(1 for f, _, _ in TABLE if f.endswith("Gen"))
    assert sum(1 for a in alloc if a >= 256) == gen, (alloc, gen)
    assert not re.search(r"\.amdhsa_private_segment_fixed_size\s+[1-9]", text)     # straight-line arithmetic in registers: no scratch
    so = build_field_probe(str(tmp_path))
    assert os.path.getsize(so) > 0


def test_the_table_is_well_formed():
    assert len(TABLE) == len(set(TABLE)) and len(TABLE) > 150
    for f, A, B in TABLE:
        fam = fm.FAMILIES[f]
        assert (B > 0) == (fam["nargs"] == 2) and (A > 0 or fam["nargs"] == 0 or f == "QDblPoint"), (f, A, B)
        if f in fm.PRODUCT_FAMILIES:
            assert fm.admits(f, A, B), (f, A, B)


# ---- which instantiations the library makes ------------------------------------------------------------------------------------------
LEAVES = {"fe_mul": "FeMul", "fe_sqr": "FeSqr", "fe2_mul_plain": "Fe2MulPlain", "fe2_mul_chain": "Fe2MulChain", "fe2_mul_signed": "Fe2MulSigned",
          "fe2_mul_asm": "Fe2MulGen", "fe2_sqr_plain": "Fe2SqrPlain", "fe2_sqr_chain": "Fe2SqrChain", "fe2_sqr_signed": "Fe2SqrSigned",
          "fe2_sqr_asm": "Fe2SqrGen", "pmul": "PMul", "pmul_const": "PMulConst", "psqr": "PSqr", "fe_add": "FeAdd", "fe_sub": "FeSub",
          "fe_neg": "FeNeg", "fe_cneg": "FeCneg", "fe2_conj": "Fe2Conj", "fe_carry": "FeCarry", "fe_sub_signed": "FeSubSigned",
          "fe_neg_signed": "FeNegSigned", "fe_cneg_signed": "FeCnegSigned", "fe_unsign": "FeUnsign", "fe_unsign_wide": "FeUnsignWide",
          "padd": "PAdd", "psub": "PSub", "pcneg": "PCneg", "pconj": "PConj", "ptighten": "PTighten", "fe_canon": "FeCanon",
          "fe_is_zero": "FeIsZero", "fe_equal": "FeEqual", "fe2_equal": "Fe2Equal", "pair_canon": "PairCanon",
          "add_affine_table": "AddAffineTable", "add_table": "AddTable", "pdbl_point": "PDblPoint", "padd_core": "PAddCore",
          "padd_affine_entry": "PAddAffineEntry", "qadd_affine_entry": "QAddAffineEntry"}
DISPATCH = ("fe2_mulx", "fe2_sqrx", "fe2_mul", "fe2_sqr", "dbl", "qdbl_point", "pmac2")


def required_entry(function, args, chain_unit):
    """the table entry that pins fq::function<args> (None: nothing of the probed families), as a (family, A, B)"""
    ints = [int(a) for a in re.findall(r"(?<![\w)])\d+\b", re.sub(r"\(fq::Mul\)\d+", "", args))]
    flav = re.search(r"\(fq::Mul\)(\d+)", args)
    if function in LEAVES:
        fam = LEAVES[function]
        n = fm.FAMILIES[fam]["nargs"]
        return (fam,) + tuple(ints[:n]) + (0,) * (2 - n)
    if function in ("fe2_mulx", "fe2_sqrx"):
        return (("Fe2Mul" if function == "fe2_mulx" else "Fe2Sqr") + fm.MUL_FLAVOURS[int(flav.group(1))],) + tuple(ints + [0])[:2]
    if function in ("fe2_mul", "fe2_sqr"):                         # the unit's MUL_FIELD: Chain where FQ_CHAIN=1, the generated product elsewhere
        return (("Fe2Mul" if function == "fe2_mul" else "Fe2Sqr") + ("Chain" if chain_unit else "Gen"),) + tuple(ints + [0])[:2]
    if function == "dbl":
        return ("Dbl" + fm.MUL_FLAVOURS[int(flav.group(1))], 0, 0) if flav else None        # dbl(const R1&) forwards to dbl<MUL_GROUP>
    if function == "qdbl_point":
        return ("QDblPoint", int(args == "true"), 0)
    if function == "pmac2":                                        # pmac2<U, V>: from pmul<U, V>, from a pmul<V, U> that swaps, or from pmul_const<U>
        U, V = ints
        swaps = lambda a, b: not fm.fits8_signed(b) and fm.fits8_signed(a)
        ways = [("PMul", U, V)] * (not swaps(U, V)) + [("PMul", V, U)] * swaps(V, U) + [("PMulConst", U, 0)] * (V == 1)
        return next((w for w in ways if w in TABLE), ways[0])
    return None


def instantiations(src):
    """[(function, template arguments)] of namespace fq in one translation unit, inlined instances included"""
    from fourq_amd import build as fb
    flags = [f for f in fb.HIPCC_FLAGS if not f.startswith("-Rpass")] + ['-DFQ_BUILD_ID="x"']
    ir = subprocess.run([fb._hipcc()] + flags + ["--cuda-device-only", "-S", "-emit-llvm", "-gline-tables-only", "-fdebug-info-for-profiling",
                         "-o", "-", os.path.join(fb.SRC_DIR, src)], check=True, capture_output=True, text=True).stdout
    names = sorted(set(re.findall(r'linkageName: "([^"]+)"', ir)))
    out = set()
    for line in fb._demangle(names):
        m = re.search(r"(?:^| )fq::(\w+)(?:<([^>]*)>)?\(", line)
        if m:
            out.add((m.group(1), m.group(2) or ""))
    return sorted(out)


def test_every_instantiation_of_the_library_has_an_id():
    from fourq_amd import build as fb
    with ThreadPoolExecutor(max_workers=4) as pool:
        per_unit = dict(zip(fb.SOURCES, pool.map(instantiations, fb.SOURCES)))
    table, missing, seen = set(TABLE), [], set()
    for src, insts in per_unit.items():
        chain = bool(re.search(r"#define FQ_CHAIN 1\b", open(os.path.join(CSRC, src)).read()))
        for function, args in insts:
            if function not in LEAVES and function not in DISPATCH:
                continue
            need = required_entry(function, args, chain)
            seen.add(function)
            if need is not None and need not in table:
                missing.append("%s: fq::%s<%s> needs E(%s, %d, %d)" % ((src, function, args) + need))
    assert not missing, "instantiations without an id in FQ_PROBE_TABLE:\n  " + "\n  ".join(missing)
    assert seen == set(LEAVES) | set(DISPATCH), sorted((set(LEAVES) | set(DISPATCH)) - seen)     # the listing still finds every family


def test_required_entry_reads_the_demangled_names():
    assert required_entry("fe2_mulx", "(fq::Mul)2, 4, 3", False) == ("Fe2MulSigned", 4, 3)
    assert required_entry("fe2_mul", "6, 3", False) == ("Fe2MulGen", 6, 3) and required_entry("fe2_mul", "6, 3", True) == ("Fe2MulChain", 6, 3)
    assert required_entry("fe2_sqrx", "(fq::Mul)0, 2", True) == ("Fe2SqrPlain", 2, 0)
    assert required_entry("fe_carry", "9", False) == ("FeCarry", 9, 0) and required_entry("add_table", "unsigned int", True) == ("AddTable", 0, 0)
    assert required_entry("dbl", "(fq::Mul)2", False) == ("DblSigned", 0, 0) and required_entry("dbl", "", False) is None
    assert required_entry("qdbl_point", "true", False) == ("QDblPoint", 1, 0)
    assert required_entry("pmac2", "4, 3", False) == ("PMul", 4, 3) and required_entry("pmac2", "1, 1", False) == ("PMul", 1, 1)
    assert required_entry("fe_mul", "9, 9", False) not in TABLE                              # an instantiation the probe lacks is reported


# ---- the frontier of the static_asserts --------------------------------------------------------------------------------------------------
def test_the_frontier_of_every_product_is_in_the_table():
    table = set(TABLE)
    for f in fm.PRODUCT_FAMILIES:
        front = fm.frontier(f)
        assert front or f == "PMulConst", f                        # pmul_const<A> admits every A <= 8 (and up to 25): no refusal to stand next to
        for A, B in front:
            assert (f, A, B) in table, (f, A, B)
    assert fm.frontier("Fe2MulSigned") == [(A, 3) for A in range(1, 9)] and fm.frontier("Fe2SqrSigned") == [(3, 0)]
    assert fm.frontier("Fe2MulGen") == [(A, 7) for A in range(1, 7)] + [(7, 6), (8, 6)] and fm.frontier("Fe2SqrGen") == [(3, 0)]
    assert fm.frontier("PMul") == [(3, B) for B in range(4, 9)] + [(A, 3) for A in range(4, 9)]
    # a product's body depends on (A, B) only through these, and both sides of each must be run:
    for fam in ("Fe2SqrSigned", "PSqr"):                           # wrap_operands_signed's / psqr's split of the factor 8
        assert {fm.fits8_signed(2 * A) for f, A, _ in TABLE if f == fam} == {True, False}
    assert {(not fm.fits8_signed(B) and fm.fits8_signed(A)) for f, A, B in TABLE if f == "PMul"} == {True, False}      # pmul's swap
    for fam in ("Fe2MulPlain", "Fe2MulChain", "Fe2MulGen"):        # fe_neg's bias (A + 1) (2^130 - 8)
        assert {A for f, A, _ in TABLE if f == fam} == set(range(1, 9))


def _asserts(text, start, end=None):
    """the conditions of the static_asserts between two markers of a header"""
    body = text[text.index(start):]
    body = body[:body.index(end, len(start))] if end else body
    return re.findall(r"static_assert\((.*?), \"", body)


def test_the_restated_asserts_match_the_headers():
    fp = open(os.path.join(CSRC, "fp127.hip.h")).read()
    pair = open(os.path.join(CSRC, "pair.hip.h")).read()
    assert "return weighted * 5 * 8 <= ((~0ull - (1ull << 41)) / (UNIT * UNIT));" in fp
    assert "return weighted * 5 * 8 <= (((1ull << 63) - (1ull << 41)) / (UNIT * UNIT));" in fp
    assert "template <int B> constexpr bool fits8_signed() { return (u64)8 * B * UNIT < (1ull << 31); }" in fp
    BIAS = "(u64)(B + 1) * (LIMB_MASK - 7) >= (u64)B * UNIT"
    assert _asserts(fp, "FQ_DEV Fe<B + 1> fe_neg(", "fe_dbl(") == [BIAS]
    assert _asserts(fp, "FQ_DEV void times8(", "// column bound") == ["(u64)8 * B * UNIT < (1ull << 32)"]
    assert _asserts(fp, "FQ_DEV Fe<1> fe_mul(", "FQ_DEV Fe<1> fe_sqr(") == ["cols_ok((u64)A * B)"]
    assert _asserts(fp, "FQ_DEV Fe<1> fe_sqr(", "// ---- GF(p^2)") == ["cols_ok((u64)A * A)", "(u64)8 * A * UNIT < (1ull << 32)"]
    for name, nxt in (("fe2_mul_chain", "fe2_mul_plain"), ("fe2_mul_plain", "// operands of the generated bodies")):
        body = fp[fp.index("FQ_DEV Fe2<1> %s(" % name):]
        body = body[:body.index(nxt)]
        assert _asserts(body, "FQ_DEV") == ["cols_ok((u64)(2 * A + 1) * B)"] and "times8(b0x8, b.re)" in body and "fe_neg(a.im)" in body
    sqc = fp[fp.index("FQ_DEV Fe2<1> fe2_sqr_chain("):fp.index("FQ_DEV Fe2<1> fe2_sqr_plain(")]
    assert _asserts(sqc, "FQ_DEV") == ["cols_ok((u64)(2 * A + 1) * (2 * A))"] and "times8(s8, s)" in sqc and "fe_sub(a.re, a.im)" in sqc
    sqp = fp[fp.index("FQ_DEV Fe2<1> fe2_sqr_plain("):fp.index("template <Mul M, int A> FQ_DEV Fe2<1> fe2_sqrx(")]
    assert "r.re = fe_mul(d, s);" in sqp and "r.im = fe_mul(t, a.im);" in sqp and "Fe<2 * A + 1> d = fe_sub(a.re, a.im);" in sqp
    assert _asserts(fp, "FQ_DEV Fe<A + B> fe_add(", "// a - b computed") == ["(u64)(A + B) * UNIT < (1ull << 32)"]
    assert _asserts(fp, "FQ_DEV Fe<A + B + 1> fe_sub(", "FQ_DEV Fe<B + 1> fe_neg(") == ["(u64)(A + B + 1) * UNIT < (1ull << 32)", BIAS]
    assert _asserts(fp, "FQ_DEV Fe<1> fe_carry(", "fe2_carry(") == ["(u64)B * UNIT + (1ull << 20) < (1ull << 32)"]
    assert _asserts(fp, "FQ_DEV Fe<B + 1> fe_cneg(", "fe2_cneg(") == [BIAS]
    assert _asserts(fp, "FQ_DEV Fe2<1> fe2_mul_signed(const Fe2<A>& a, const Fe2<B>& b) {", "FQ_DEV Fe2<1> fe2_sqr_signed(") == [
        "cols_ok_signed((u64)2 * A * B)", "fits8_signed<B>()"]
    assert _asserts(fp, "FQ_DEV Fe2<1> fe2_sqr_signed(const Fe2<A>& a) {", "#undef FQ_OPAQUE") == [
        "(u64)2 * A * UNIT < (1ull << 31)", "cols_ok_signed((u64)(2 * A) * (2 * A))"]
    assert _asserts(fp, "FQ_DEV void wrap_operands_signed(", "#define FQ_OPAQUE") == ["(u64)4 * A * UNIT < (1ull << 31) && (u64)2 * B * UNIT < (1ull << 31)"]
    assert "wrap_operands_signed(dw, s8, d, s);" in fp and "wrap_operands_signed(tw, i8, t, a.im);" in fp and "if constexpr (fits8_signed<B>()) {" in fp
    for name in ("fe_unsign(", "fe_unsign_wide("):
        body = fp[fp.index("FQ_DEV Fe<%s> %s" % ("1" if name == "fe_unsign(" else "2 * B + 1", name)):]
        assert _asserts(body[:body.index("return")], "FQ_DEV") == [BIAS, "(u64)(2 * B + 1) * UNIT + (1ull << 20) < (1ull << 32)"]
    assert _asserts(fp, "FQ_DEV Fe<A + B> fe_sub_signed(", "fe_neg_signed(") == ["(u64)(A + B) * UNIT < (1ull << 31)"]
    assert _asserts(pair, "FQ_DEV PF<1> pmac2(", "// a * b.") == ["cols_ok_signed((u64)2 * U * V)", "fits8_signed<V>()"]
    assert "if constexpr (!fits8_signed<B>() && fits8_signed<A>()) {" in pair and "return pmac2<A, B>(a.l, v.l, w.l, z.l);" in pair
    assert "return pmac2<A, 1>(a.l, v, w.l, z);" in pair
    assert _asserts(pair, "FQ_DEV PF<1> psqr(", "#undef FQ_POPAQUE") == [
        "(u64)2 * A * UNIT < (1ull << 31)", "cols_ok_signed((u64)(2 * A) * (2 * A))", "!WIDE || ((u64)4 * 2 * A * UNIT < (1ull << 31))"]
    assert "constexpr bool WIDE = !fits8_signed<2 * A>();" in pair
    assert _asserts(pair, "FQ_DEV PF<A + B> padd(", "pdbl(") == ["(u64)(A + B) * UNIT < (1ull << 31)"] * 2       # padd and psub
    # the restatement at its boundaries
    lim = ((1 << 63) - (1 << 41)) // (fm.UNIT * fm.UNIT)
    assert all(fm.cols_ok_signed(w) == (w * 40 <= lim) for w in range(1, 120)) and fm.cols_ok_signed(51) and not fm.cols_ok_signed(52)
    assert fm.cols_ok(102) and not fm.cols_ok(103)
    assert fm.fits8_signed(3) and not fm.fits8_signed(4) and fm.bias_ok(2047) and not fm.bias_ok(2048)
    assert not fm.admits("Fe2MulSigned", 15, 3) and not fm.admits("Fe2MulSigned", 63, 1) and not fm.admits("Fe2SqrSigned", 4)
    assert [A for A in range(1, 9) if fm.admits("Fe2SqrGen", A)] == [1, 2, 3] and fm.admits("PMulConst", 25) and not fm.admits("PMulConst", 26)


# ---- the model keeps the contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(fm.FAMILIES))
def test_the_model_meets_the_contract_on_every_vector(family):
    entries = [e for e in TABLE if e[0] == family]
    assert entries, family
    for entry in entries:
        vecs = fm.vectors(entry)
        assert len(vecs) >= 4 + 256
        for k, (pattern, v, mask) in enumerate(vecs):
            try:
                out = fm.model_outputs(entry, v, mask)
            except fm.ModelOverflow as exc:
                raise AssertionError("%s vector %d (%s, mask %x): %s" % (fm.entry_name(entry), k, pattern, mask, exc))
            bad = fm.check_outputs(entry, out, fm.expected(entry, v, mask))
            assert bad is None, "%s vector %d (%s, mask %x): %s" % (fm.entry_name(entry), k, pattern, mask, bad)


def test_the_contract_bites():
    """check_outputs refuses a wrong residue, a right residue in limbs outside the promise, a wrong canonical word and a wrong verdict"""
    entry = ("Fe2MulSigned", 4, 3)
    _, v, mask = fm.vectors(entry)[0]
    want, good = fm.expected(entry, v, mask), fm.model_outputs(entry, v, mask)
    assert fm.check_outputs(entry, good, want) is None
    off = {"r": [good["r"][0] + 1] + good["r"][1:]}
    assert "residue" in fm.check_outputs(entry, off, want)
    loose = {"r": [good["r"][0] + (1 << 26), good["r"][1] - 1] + good["r"][2:]}            # the same residue, limb 0 not below 2^26
    assert fm.res(loose["r"]) == want["r"] and "outside" in fm.check_outputs(entry, loose, want)
    edge = [0, fm.UNIT - 1, 0, 0, 0, 0, -(fm.UNIT - 1), 0, 0, fm.M26]                     # a product's widest shape passes, one more does not
    assert fm.check_outputs(entry, {"r": edge}, {"r": fm.res(edge)}) is None
    for i, x in ((1, fm.UNIT), (6, -fm.UNIT), (9, 1 << 26), (2, -1)):
        wide = edge[:i] + [x] + edge[i + 1:]
        assert "outside" in fm.check_outputs(entry, {"r": wide}, {"r": fm.res(wide)})
    tight = ("FeUnsign", 4, 0)
    _, v, mask = fm.vectors(tight)[1]                              # all limbs at -4 UNIT
    neg = {"r": [x - k for x, k in zip(fm.model_outputs(tight, v, mask)["r"], (1 << 26, -1, 0, 0, 0))]}
    assert "outside" in fm.check_outputs(tight, neg, fm.expected(tight, v, mask))            # a negative limb where the type promises none
    assert fm.check_outputs(("FeCanon", 2, 0), {"r": fm.P}, {"r": 0}) and fm.check_outputs(("FeEqual", 1, 1), {"r": 1}, {"r": 0})
    rows = fm.pack(entry, [("x", v0, 0) for _, v0, _ in fm.vectors(entry)[:3]])
    assert fm.unpack(entry, rows)[1][0]["r"] == fm.vectors(entry)[1][1]["a"]                 # records round-trip, signed limbs included


def test_vectors_are_the_same_every_time_and_reach_the_corners():
    entry = ("Fe2MulSigned", 4, 3)
    vecs = fm.vectors(entry)
    assert vecs == fm.vectors(entry)
    assert vecs[0][1]["a"] == [4 * fm.UNIT] * 10 and vecs[1][1]["b"] == [-3 * fm.UNIT] * 10
    assert len({tuple(v["a"] + v["b"]) for p, v, _ in vecs if p.startswith("combo")}) == 16
    zero = fm.zero_class(3, False, __import__("random").Random(1))
    assert any(l == [3 * fm.M26] * 4 + [3 * ((1 << 23) - 1)] for _, d, l in zero if d == 0)
    assert any(l == [3 * (fm.M26 - 7)] + [3 * fm.M26] * 4 for _, d, l in zero if d == 0) and {d for _, d, _ in zero} == {0, 1, -1}
    rows = fm.pack(("PMul", 1, 1), fm.vectors(("PMul", 1, 1))[:2])
    assert len(rows) == 4 and rows[0][:5] == [fm.UNIT] * 5 and rows[1][10:15] == [fm.UNIT] * 5


@pytest.mark.parametrize("entry", [("Fe2MulSigned", 15, 3), ("Fe2MulSigned", 63, 1), ("Fe2SqrSigned", 4, 0), ("PSqr", 4, 0)])
def test_the_model_overflows_where_the_asserts_refuse(entry):
    assert not fm.admits(*entry)
    with pytest.raises(fm.ModelOverflow):
        for _, v, mask in fm.vectors(entry):
            fm.model_outputs(entry, v, mask)
