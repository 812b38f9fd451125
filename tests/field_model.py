"""The limb arithmetic hipcc compiles from fp127.hip.h / pair.hip.h / curve.hip.h, restated on Python integers: the entries of
tests/hip/field_flavour_probe.hip (FQ_PROBE_TABLE, read from that file's text), their corner inputs, what they must deliver, and a model.

What a vector must deliver (check_outputs) is stated on RESIDUES and BOUNDS only: value(l) = sum l_i 2^(26 i) mod p = 2^127 - 1, the
operation on the input residues computed with curve4q_oracle's field functions, and every output limb inside what the result type
promises.  The model is a third party to that: it restates the headers' column loops on unbounded integers and raises ModelOverflow
where a 32-bit operand or a 64-bit accumulator would leave its range, so tests/test_field_probe.py can show on the CPU that the C++
as written meets the contract on the very vectors the MI355X is given (tests/test_gpu_field_corners.py)."""
import os
import random
import re
import sys
import zlib

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools", "asmgen"))
import bounds as bd                # noqa: E402
import curve4q_oracle as o         # noqa: E402

PROBE_SRC = os.path.join(ROOT, "tests", "hip", "field_flavour_probe.hip")
P = (1 << 127) - 1
M26, M32, UNIT = (1 << 26) - 1, (1 << 32) - 1, bd.UNIT
WORDS, ENTRY_AT, MASK_AT = 128, 64, 120
EXTRA, SAMPLE = 256, 64             # random-extreme vectors per entry; max / min combinations kept when there are more


class ModelOverflow(Exception):
    """a 32-bit operand or a 64-bit accumulator of the C++ as written would wrap"""


def _u32(x):
    if not 0 <= x <= M32:
        raise ModelOverflow("u32 %d" % x)
    return x


def _i32(x):
    if not -(1 << 31) <= x < (1 << 31):
        raise ModelOverflow("i32 %d" % x)
    return x


def _u64(x):
    if not 0 <= x < (1 << 64):
        raise ModelOverflow("u64 %d" % x)
    return x


def _i64(x):
    if not -(1 << 63) <= x < (1 << 63):
        raise ModelOverflow("i64 %d" % x)
    return x


def value(l):
    return sum(x << (26 * i) for i, x in enumerate(l))


def bias(k):
    return [bd.bias_limb(k, i) for i in range(5)]


# ---- the headers' static_asserts, restated (tests/test_field_probe.py checks their text) ------------------------------------------------
def cols_ok(weighted):
    return bd.cols_ok(weighted)


def cols_ok_signed(weighted):
    return weighted * 5 * 8 <= ((1 << 63) - (1 << 41)) // (UNIT * UNIT)


def fits8_signed(B):
    return 8 * B * UNIT < (1 << 31)


def bias_ok(B):
    return (B + 1) * (M26 - 7) >= B * UNIT


def admits(family, A, B=0):
    """do the static_asserts on the way through `family`<A, B> hold (the helpers it calls included)"""
    if family == "FeMul":
        return cols_ok(A * B) and 8 * B * UNIT < (1 << 32)
    if family == "FeSqr":
        return cols_ok(A * A) and 8 * A * UNIT < (1 << 32)
    if family in ("Fe2MulPlain", "Fe2MulChain", "Fe2MulGen"):      # times8 of b, fe_neg of a.im
        return cols_ok((2 * A + 1) * B) and 8 * B * UNIT < (1 << 32) and bias_ok(A)
    if family in ("Fe2SqrPlain", "Fe2SqrChain", "Fe2SqrGen"):      # fe_add, fe_sub, fe_dbl; times8 of s and of a.im
        return (cols_ok((2 * A + 1) * (2 * A)) and 8 * 2 * A * UNIT < (1 << 32) and (2 * A + 1) * UNIT < (1 << 32) and bias_ok(A))
    if family == "Fe2MulSigned":
        return cols_ok_signed(2 * A * B) and fits8_signed(B)
    if family == "Fe2SqrSigned":       # wrap_operands_signed<2A, 2A> and <2A, A>
        wrap = all(fits8_signed(b) or (4 * a * UNIT < (1 << 31) and 2 * b * UNIT < (1 << 31)) for a, b in ((2 * A, 2 * A), (2 * A, A)))
        return 2 * A * UNIT < (1 << 31) and cols_ok_signed(4 * A * A) and wrap
    if family == "PMul":
        if not fits8_signed(B) and fits8_signed(A):
            A, B = B, A
        return cols_ok_signed(2 * A * B) and fits8_signed(B)
    if family == "PMulConst":
        return cols_ok_signed(2 * A)
    if family == "PSqr":
        wide = not fits8_signed(2 * A)
        return 2 * A * UNIT < (1 << 31) and cols_ok_signed(4 * A * A) and (not wide or 4 * 2 * A * UNIT < (1 << 31))
    raise KeyError(family)


PRODUCT_FAMILIES = ("FeMul", "FeSqr", "Fe2MulPlain", "Fe2MulChain", "Fe2MulSigned", "Fe2MulGen", "Fe2SqrPlain", "Fe2SqrChain",
                    "Fe2SqrSigned", "Fe2SqrGen", "PMul", "PMulConst", "PSqr")
FRONTIER_CAP = 8


def frontier(family):
    """the admitted (A, B) with A, B <= 8 next to a refusal: (A + 1, B) or (A, B + 1) is refused"""
    two = FAMILIES[family]["nargs"] == 2
    out = []
    for A in range(1, FRONTIER_CAP + 1):
        for B in (range(1, FRONTIER_CAP + 1) if two else (0,)):
            if admits(family, A, B) and (not admits(family, A + 1, B) or (two and not admits(family, A, B + 1))):
                out.append((A, B))
    return out


# ---- the model: unsigned flavour ----------------------------------------------------------------------------------------------------------
def fe_add(a, b):
    return [_u32(x + y) for x, y in zip(a, b)]


def fe_neg(b, B):
    return [_u32(k - x) for k, x in zip(bias(B + 1), b)]


def fe_sub(a, b, B):
    return [_u32(x + y) for x, y in zip(a, fe_neg(b, B))]


def fe_cneg(x, B, mask):               # (x ^ mask) + ((bias + 1) & mask): wraps through 2^32 by design where mask is set
    return [((v ^ mask) + ((k + 1) & mask)) & M32 for k, v in zip(bias(B + 1), x)]


def fe_carry(a):
    a = [_u32(x) for x in a]
    t1 = _u32(a[1] + (a[0] >> 26))
    t2 = _u32(a[2] + (t1 >> 26))
    t3 = _u32(a[3] + (t2 >> 26))
    t4 = _u32(a[4] + (t3 >> 26))
    t0 = _u32((a[0] & M26) + _u32((t4 >> 26) << 3))
    return [t0 & M26, _u32((t1 & M26) + (t0 >> 26)), t2 & M26, t3 & M26, t4 & M26]


def times8(b):
    return [_u32(x << 3) for x in b]


def _finish(l, top):
    w = _u64((_u64(top << 3)) + l[0])
    return [w & M26, _u32(l[1] + _u32(w >> 26)), l[2], l[3], l[4]]


def _mac(pairs):
    """fe_mac2 / the column loops of fe2_mul_chain: sum of GF(p) products a * b, (a, b, 8b) each, columns in order with the carry"""
    l, acc = [], 0
    for K in range(5):
        for a, b, b8 in pairs:
            for i in range(5):
                j = K - i
                acc = _u64(acc + _u32(a[i]) * _u32(b[j] if j >= 0 else b8[j + 5]))
        l.append(acc & M26)
        acc >>= 26
    return _finish(l, acc)


def fe_mul(a, b):
    return _mac([(a, b, times8(b))])


def fe_sqr(x):
    x = [_u32(v) for v in x]
    d, e = [_u32(v << 1) for v in x], [_u32(v << 3) for v in x]
    cols = [[(x[0], x[0]), (d[1], e[4]), (d[2], e[3])], [(d[0], x[1]), (d[2], e[4]), (x[3], e[3])], [(d[0], x[2]), (x[1], x[1]), (d[3], e[4])],
            [(d[0], x[3]), (d[1], x[2]), (x[4], e[4])], [(d[0], x[4]), (d[1], x[3]), (x[2], x[2])]]
    l, acc = [], 0
    for col in cols:
        acc = _u64(acc + sum(p * q for p, q in col))
        l.append(acc & M26)
        acc >>= 26
    return _finish(l, acc)


def fe2_mul_u(a, b, A):                # fe2_mul_plain / fe2_mul_chain / fe2_mul_asm: the same sums, column by column
    are, aim, bre, bim = a[:5], a[5:], b[:5], b[5:]
    b0, b1, na1 = times8(bre), times8(bim), fe_neg(aim, A)
    return _mac([(are, bre, b0), (na1, bim, b1)]) + _mac([(are, bim, b1), (aim, bre, b0)])


def fe2_sqr_u(a, A):
    re_, im = a[:5], a[5:]
    s, d, t = fe_add(re_, im), fe_sub(re_, im, A), fe_add(re_, re_)
    return fe_mul(d, s) + fe_mul(t, im)


def fe2_add(a, b):
    return fe_add(a, b)


def fe2_sub(a, b, B):
    return fe_sub(a[:5], b[:5], B) + fe_sub(a[5:], b[5:], B)


# ---- the model: signed flavour and the pair lanes -------------------------------------------------------------------------------------
def s_add(a, b):
    return [_i32(x + y) for x, y in zip(a, b)]


def s_sub(a, b):
    return [_i32(x - y) for x, y in zip(a, b)]


def s_neg(a):
    return [_i32(-x) for x in a]


def s_cneg(a, mask):                   # (x ^ mask) - mask
    return s_neg(a) if mask else list(a)


def _shl(a, k):
    return [_i32(x << k) for x in a]


def _finish_s(l, top):
    w = _i64(_i64(top * 8) + l[0])
    return [w & M26, _i32(l[1] + _i32(w >> 26)), l[2], l[3], l[4]]


def _mac_s(main, side=None):
    """signed columns: main(K) / side(K) list the (x, y) of each multiply-add in the order the C++ issues them; `side` is pmac2's and
    psqr's second chain, which starts from zero in every column and is added once"""
    l, acc = [], 0
    for K in range(5):
        for x, y in main(K):
            acc = _i64(acc + _i32(x) * _i32(y))
        if side is not None:
            s = 0
            for x, y in side(K):
                s = _i64(s + _i32(x) * _i32(y))
            acc = _i64(acc + s)
        l.append(acc & M26)
        acc >>= 26
    return _finish_s(l, acc)


def _terms(a, b, b8, aw=None):
    aw = a if aw is None else aw
    return lambda K: [((a[i] if K - i >= 0 else aw[i]), (b[K - i] if K - i >= 0 else b8[K - i + 5])) for i in range(5)]


def _interleave(f, g):
    return lambda K: [t for pair in zip(f(K), g(K)) for t in pair]


def fe2_mul_signed(a, b):
    are, aim, bre, bim = a[:5], a[5:], b[:5], b[5:]
    b0, b1, na1 = _shl(bre, 3), _shl(bim, 3), s_neg(aim)
    return (_mac_s(_interleave(_terms(are, bre, b0), _terms(na1, bim, b1))) +
            _mac_s(_interleave(_terms(are, bim, b1), _terms(aim, bre, b0))))


def wrap_operands_signed(a, b, B):
    return (list(a), _shl(b, 3)) if fits8_signed(B) else (_shl(a, 2), _shl(b, 1))


def fe2_sqr_signed(a, A):
    re_, im = a[:5], a[5:]
    s, d, t = s_add(re_, im), s_sub(re_, im), s_add(re_, re_)
    dw, s8 = wrap_operands_signed(d, s, 2 * A)
    tw, i8 = wrap_operands_signed(t, im, A)
    return _mac_s(_terms(d, s, s8, dw)) + _mac_s(_terms(t, im, i8, tw))


def fe_unsign_wide(a, B):
    return [_u32(x + k) for x, k in zip(a, bias(B + 1))]


def fe_unsign(a, B):
    return fe_carry(fe_unsign_wide(a, B))


def pmac2(u, v, w, z):
    return _mac_s(_terms(u, v, _shl(v, 3)), _terms(w, z, _shl(z, 3)))


def pmul(a, b, A, B):
    """both lanes of a pair: the even lane's half (re) and the odd lane's (im)"""
    if not fits8_signed(B) and fits8_signed(A):
        a, b = b, a
    are, aim, bre, bim = a[:5], a[5:], b[:5], b[5:]
    return pmac2(are, bre, s_neg(aim), bim) + pmac2(aim, bre, are, bim)


def psqr(a, A):
    re_, im = a[:5], a[5:]
    wide = not fits8_signed(2 * A)
    out = []
    for u, v in ((s_add(im, re_), s_sub(re_, im)), (s_add(re_, re_), im)):       # even lane | odd lane
        vw, uw = _shl(v, 1 if wide else 3), (_shl(u, 2) if wide else u)
        terms = _terms(u, v, vw, uw)
        out += _mac_s(lambda K: terms(K)[0::2], lambda K: terms(K)[1::2])
    return out


def p_add(a, b):
    return s_add(a, b)


def p_sub(a, b):
    return s_sub(a, b)


# ---- the model: the group law, formula by formula as the headers write it ------------------------------------------------------------
def dbl_u(X, Y, Z):                    # dbl<Mul::Plain / Chain>
    A, B = fe2_sqr_u(X, 1), fe2_sqr_u(Y, 1)
    zz = fe2_sqr_u(Z, 1)
    C, D = fe2_add(zz, zz), fe2_add(A, B)
    E = fe2_sub(fe2_sqr_u(fe2_add(X, Y), 2), D, 2)
    F = fe2_sub(B, A, 1)
    G = fe2_sub(C, F, 3)
    return {"X": fe2_mul_u(E, G, 4), "Z": fe2_mul_u(F, G, 3), "Y": fe2_mul_u(F, D, 3), "Ta": E, "Tb": D}


def dbl_s(X, Y, Z):                    # dbl<Mul::Signed>
    A, B = fe2_sqr_signed(X, 1), fe2_sqr_signed(Y, 1)
    zz = fe2_sqr_signed(Z, 1)
    C, D = s_add(zz, zz), s_add(A, B)
    E = s_sub(fe2_sqr_signed(s_add(X, Y), 2), D)
    F = s_sub(B, A)
    G = s_sub(C, F)
    return {"X": fe2_mul_signed(G, E), "Z": fe2_mul_signed(G, F), "Y": fe2_mul_signed(D, F), "Ta": E, "Tb": D}


def add_affine_table(v, mask):
    T = fe2_mul_signed(v["Ta"], v["Tb"])
    N1, D1 = s_add(v["X"], v["Y"]), s_sub(v["Y"], v["X"])
    tN, tD = (v["e1"], v["e0"]) if mask else (v["e0"], v["e1"])
    A, B = fe2_mul_signed(D1, tD), fe2_mul_signed(N1, tN)
    C = fe2_mul_signed(s_cneg(v["e2"], mask), T)
    D = s_add(v["Z"], v["Z"])
    E, G, H, F = s_sub(B, A), s_add(D, C), s_add(B, A), s_sub(D, C)
    return {"X": fe2_mul_signed(E, F), "Z": fe2_mul_signed(G, F), "Y": fe2_mul_signed(G, H), "Ta": E, "Tb": H}


def add_table(v, mask):                # MUL_GROUP products on unsigned limbs
    T = fe2_mul_u(v["Ta"], v["Tb"], 4)
    N1, D1 = fe2_add(v["X"], v["Y"]), fe2_sub(v["Y"], v["X"], 1)
    tN, tD = (v["e1"], v["e0"]) if mask else (v["e0"], v["e1"])
    A, B = fe2_mul_u(D1, tD, 3), fe2_mul_u(N1, tN, 2)
    C = fe2_mul_u(fe_cneg(v["e3"][:5], 1, mask) + fe_cneg(v["e3"][5:], 1, mask), T, 2)
    D = fe2_mul_u(v["e2"], v["Z"], 1)
    E, F, G, H = fe2_sub(B, A, 1), fe2_sub(D, C, 1), fe2_add(D, C), fe2_add(B, A)
    return {"X": fe2_mul_u(E, F, 3), "Z": fe2_mul_u(G, F, 2), "Y": fe2_mul_u(G, H, 2), "Ta": E, "Tb": H}


def pdbl_point(X, Y, Z, with_t=None):
    """pdbl_point; with_t False / True: qdbl_point<WITH_T>, the same products two at a time -- qsel hands both pairs the WIDER of its two
    types, so Z is squared as a PF<2> and F multiplied as a PF<3> -- and T = D * E too where WITH_T"""
    quad = with_t is not None
    A, B = psqr(X, 1), psqr(Y, 1)
    zz = psqr(Z, 2 if quad else 1)
    C, D = s_add(zz, zz), s_add(A, B)
    E = s_sub(psqr(s_add(X, Y), 2), D)
    F = s_sub(B, A)
    G = s_sub(C, F)
    if not quad:
        return {"X": pmul(G, E, 4, 3), "Z": pmul(G, F, 4, 2), "Y": pmul(D, F, 2, 2), "Ta": E, "Tb": D}
    r = {"X": pmul(G, E, 4, 3), "Z": pmul(G, F, 4, 3), "Ta": E, "Tb": D}
    r["Y"] = pmul(D, F, 2, 3) if with_t else pmul(D, F, 2, 2)
    r["T"] = pmul(D, E, 2, 3) if with_t else r["Y"]
    return r


def padd_core(v):
    A, B = pmul(v["pD"], v["qD"], 2, 2), pmul(v["pN"], v["qN"], 2, 2)
    C, D = pmul(v["qF"], v["pF"], 1, 1), pmul(v["qE"], v["pE"], 2, 1)
    E, F, G, H = s_sub(B, A), s_sub(D, C), s_add(D, C), s_add(B, A)
    return {"X": pmul(E, F, 2, 2), "Y": pmul(G, H, 2, 2), "Z": pmul(F, G, 2, 2), "Ta": E, "Tb": H}


def padd_affine(v, mask, quad):
    """padd_affine_entry (T = Ta * Tb first) / qadd_affine_entry (T in, T' = E * H out; qsel widens both operands of the last level)"""
    T = v["T"] if quad else pmul(v["Ta"], v["Tb"], 3, 2)
    sN, sD = (v["aD"], v["aN"]) if mask else (v["aN"], v["aD"])
    A, B = pmul(s_sub(v["Y"], v["X"]), sD, 2, 1), pmul(s_add(v["X"], v["Y"]), sN, 2, 1)
    C = pmul(s_cneg(v["aF"], mask), T, 1, 1)
    D = s_add(v["Z"], v["Z"])
    E, H, F, G = s_sub(B, A), s_add(B, A), s_sub(D, C), s_add(D, C)
    if quad:
        return {"X": pmul(E, F, 3, 3), "Y": pmul(G, H, 3, 3), "Z": pmul(F, G, 3, 3), "T": pmul(E, H, 3, 3), "Ta": E, "Tb": H}
    return {"X": pmul(E, F, 2, 3), "Y": pmul(G, H, 3, 2), "Z": pmul(F, G, 3, 3), "Ta": E, "Tb": H}


# ---- canonical form ---------------------------------------------------------------------------------------------------------------------
def fe_canon(a):
    t = fe_carry(a)
    l = [_u32(t[0] + (t[4] >> 23)), t[1], t[2], t[3], t[4] & 0x7fffff]
    for _ in range(2):
        for i in range(4):
            l[i + 1] = _u32(l[i + 1] + (l[i] >> 26))
            l[i] &= M26
        if _ == 0:
            l[0] = _u32(l[0] + (l[4] >> 23))
            l[4] &= 0x7fffff
    if l == [M26] * 4 + [0x7fffff]:
        l = [0] * 5
    lo = (l[0] | l[1] << 26 | l[2] << 52) & ((1 << 64) - 1)
    hi = (l[2] >> 12 | l[3] << 14 | l[4] << 40) & ((1 << 64) - 1)
    return lo | hi << 64


# ---- the reference: residues through curve4q_oracle -----------------------------------------------------------------------------------
def res(l):
    """residue of a five-limb element, residue pair of a ten-limb one"""
    return value(l) % P if len(l) == 5 else (value(l[:5]) % P, value(l[5:]) % P)


def _r1(t):
    return dict(zip(("X", "Y", "Z", "Ta", "Tb"), t))


def _ref_add_affine(r, mask, T):
    N, D, F = (r["aD"], r["aN"], o.f2_neg(r["aF"])) if mask else (r["aN"], r["aD"], r["aF"])
    return o.ADD_core((o.f2_add(r["X"], r["Y"]), o.f2_sub(r["Y"], r["X"]), r["Z"], T), (N, D, o.F2_TWO, F))


# ---- the families -------------------------------------------------------------------------------------------------------------------------
# operands: (name, kind, bound); kinds: "fe" five limbs, "fe2" ten, "pf" ten at element level (re for the even lane, im for the odd one),
# "c2" a GF(p^2) constant whole in every lane's record, "entry" a table entry's coordinate (non-negative tight limbs) at ENTRY_AT + 12c.
# outs: (name, word, kind, promise); kinds as above plus "words" (a canonical 128-bit value), "pwords" (one per lane) and "flag";
# promises: "prod" (a product's shape), "tight" (non-negative, <= UNIT), ("lazy", B) (within B * UNIT in the family's sign convention)
def _fam(cpp, nargs, signed, lanes, operands, outs, model, ref, mask=False, zero=None):
    return dict(cpp=cpp, nargs=nargs, signed=signed, lanes=lanes, operands=operands, outs=outs, model=model, ref=ref, mask=mask, zero=zero)


def _bin(kind):
    return lambda A, B: [("a", kind, A), ("b", kind, B)]


def _un(kind):
    return lambda A, B: [("a", kind, A)]


def _out(kind, promise):
    return lambda A, B: [("r", 0, kind, promise(A, B) if callable(promise) else promise)]


R1_OUT = lambda A, B: [("X", 0, "fe2", "prod"), ("Y", 10, "fe2", "prod"), ("Z", 20, "fe2", "prod"), ("Ta", 30, "fe2", ("lazy", 4)), ("Tb", 40, "fe2", ("lazy", 2))]
PR1_OUT = lambda A, B: [("X", 0, "pf", "prod"), ("Y", 10, "pf", "prod"), ("Z", 20, "pf", "prod"), ("Ta", 30, "pf", ("lazy", 3)), ("Tb", 40, "pf", ("lazy", 2))]
PR1_T_OUT = lambda A, B: PR1_OUT(A, B) + [("T", 50, "pf", "prod")]
XYZ = lambda kind: lambda A, B: [("X", kind, 1), ("Y", kind, 1), ("Z", kind, 1)]
R1_IN = lambda kind, ta: [("X", kind, 1), ("Y", kind, 1), ("Z", kind, 1), ("Ta", kind, ta), ("Tb", kind, 2)]
_dbl_ref = lambda A, B, r, m: _r1(o.DBL((r["X"], r["Y"], r["Z"])))
_m1 = lambda f: (lambda A, B, v, m: {"r": f(A, B, v, m)})
_r1f = lambda f: (lambda A, B, r, m: {"r": f(A, B, r, m)})

FAMILIES = {
    # ---- products and squares
    "FeMul": _fam(["fe_mul"], 2, False, 1, _bin("fe"), _out("fe", "prod"), _m1(lambda A, B, v, m: fe_mul(v["a"], v["b"])), _r1f(lambda A, B, r, m: o.fp_mul(r["a"], r["b"]))),
    "FeSqr": _fam(["fe_sqr"], 1, False, 1, _un("fe"), _out("fe", "prod"), _m1(lambda A, B, v, m: fe_sqr(v["a"])), _r1f(lambda A, B, r, m: o.fp_sqr(r["a"]))),
    "PMul": _fam(["pmul"], 2, True, 2, _bin("pf"), _out("pf", "prod"), _m1(lambda A, B, v, m: pmul(v["a"], v["b"], A, B)), _r1f(lambda A, B, r, m: o.f2_mul(r["a"], r["b"]))),
    "PMulConst": _fam(["pmul_const"], 1, True, 2, lambda A, B: [("a", "pf", A), ("b", "c2", 1)], _out("pf", "prod"),
                      _m1(lambda A, B, v, m: pmul(v["a"], v["b"], A, 1)), _r1f(lambda A, B, r, m: o.f2_mul(r["a"], r["b"]))),
    "PSqr": _fam(["psqr"], 1, True, 2, _un("pf"), _out("pf", "prod"), _m1(lambda A, B, v, m: psqr(v["a"], A)), _r1f(lambda A, B, r, m: o.f2_sqr(r["a"]))),
    # ---- lazy operations and exits
    "FeAdd": _fam(["fe_add"], 2, False, 1, _bin("fe"), _out("fe", lambda A, B: ("lazy", A + B)), _m1(lambda A, B, v, m: fe_add(v["a"], v["b"])), _r1f(lambda A, B, r, m: o.fp_add(r["a"], r["b"]))),
    "FeSub": _fam(["fe_sub"], 2, False, 1, _bin("fe"), _out("fe", lambda A, B: ("lazy", A + B + 1)), _m1(lambda A, B, v, m: fe_sub(v["a"], v["b"], B)), _r1f(lambda A, B, r, m: o.fp_sub(r["a"], r["b"]))),
    "FeNeg": _fam(["fe_neg"], 1, False, 1, _un("fe"), _out("fe", lambda A, B: ("lazy", A + 1)), _m1(lambda A, B, v, m: fe_neg(v["a"], A)), _r1f(lambda A, B, r, m: o.fp_neg(r["a"]))),
    "FeCneg": _fam(["fe_cneg"], 1, False, 1, _un("fe"), _out("fe", lambda A, B: ("lazy", A + 1)), _m1(lambda A, B, v, m: fe_cneg(v["a"], A, m)),
                   _r1f(lambda A, B, r, m: o.fp_neg(r["a"]) if m else r["a"]), mask=True),
    "Fe2Conj": _fam(["fe2_conj"], 1, False, 1, _un("fe2"), _out("fe2", lambda A, B: ("lazy", A + 1)), _m1(lambda A, B, v, m: v["a"][:5] + fe_neg(v["a"][5:], A)), _r1f(lambda A, B, r, m: o.f2_conj(r["a"]))),
    "FeCarry": _fam(["fe_carry"], 1, False, 1, _un("fe"), _out("fe", "tight"), _m1(lambda A, B, v, m: fe_carry(v["a"])), _r1f(lambda A, B, r, m: r["a"])),
    "FeSubSigned": _fam(["fe_sub_signed"], 2, True, 1, _bin("fe"), _out("fe", lambda A, B: ("lazy", A + B)), _m1(lambda A, B, v, m: s_sub(v["a"], v["b"])), _r1f(lambda A, B, r, m: o.fp_sub(r["a"], r["b"]))),
    "FeNegSigned": _fam(["fe_neg_signed"], 1, True, 1, _un("fe"), _out("fe", lambda A, B: ("lazy", A)), _m1(lambda A, B, v, m: s_neg(v["a"])), _r1f(lambda A, B, r, m: o.fp_neg(r["a"]))),
    "FeCnegSigned": _fam(["fe_cneg_signed"], 1, True, 1, _un("fe"), _out("fe", lambda A, B: ("lazy", A)), _m1(lambda A, B, v, m: s_cneg(v["a"], m)),
                         _r1f(lambda A, B, r, m: o.fp_neg(r["a"]) if m else r["a"]), mask=True),
    "FeUnsign": _fam(["fe_unsign"], 1, True, 1, _un("fe"), _out("fe", "tight"), _m1(lambda A, B, v, m: fe_unsign(v["a"], A)), _r1f(lambda A, B, r, m: r["a"])),
    "FeUnsignWide": _fam(["fe_unsign_wide"], 1, True, 1, _un("fe"), _out("fe", lambda A, B: ("ulazy", 2 * A + 1)), _m1(lambda A, B, v, m: fe_unsign_wide(v["a"], A)), _r1f(lambda A, B, r, m: r["a"])),
    "PAdd": _fam(["padd"], 2, True, 2, _bin("pf"), _out("pf", lambda A, B: ("lazy", A + B)), _m1(lambda A, B, v, m: s_add(v["a"], v["b"])), _r1f(lambda A, B, r, m: o.f2_add(r["a"], r["b"]))),
    "PSub": _fam(["psub"], 2, True, 2, _bin("pf"), _out("pf", lambda A, B: ("lazy", A + B)), _m1(lambda A, B, v, m: s_sub(v["a"], v["b"])), _r1f(lambda A, B, r, m: o.f2_sub(r["a"], r["b"]))),
    "PCneg": _fam(["pcneg"], 1, True, 2, _un("pf"), _out("pf", lambda A, B: ("lazy", A)), _m1(lambda A, B, v, m: s_cneg(v["a"], m)),
                  _r1f(lambda A, B, r, m: o.f2_neg(r["a"]) if m else r["a"]), mask=True),
    "PConj": _fam(["pconj"], 1, True, 2, _un("pf"), _out("pf", lambda A, B: ("lazy", A)), _m1(lambda A, B, v, m: v["a"][:5] + s_neg(v["a"][5:])), _r1f(lambda A, B, r, m: o.f2_conj(r["a"]))),
    "PTighten": _fam(["ptighten"], 1, True, 2, _un("pf"), _out("pf", "tight"), _m1(lambda A, B, v, m: fe_unsign(v["a"][:5], A) + fe_unsign(v["a"][5:], A)), _r1f(lambda A, B, r, m: r["a"])),
    # ---- canonical form and verdicts
    "FeCanon": _fam(["fe_canon"], 1, False, 1, _un("fe"), _out("words", None), _m1(lambda A, B, v, m: fe_canon(v["a"])), _r1f(lambda A, B, r, m: r["a"]), zero="one"),
    "FeIsZero": _fam(["fe_is_zero"], 1, False, 1, _un("fe"), _out("flag", None), _m1(lambda A, B, v, m: int(fe_canon(v["a"]) == 0)), _r1f(lambda A, B, r, m: int(r["a"] == 0)), zero="one"),
    "FeEqual": _fam(["fe_equal"], 2, False, 1, _bin("fe"), _out("flag", None), _m1(lambda A, B, v, m: int(fe_canon(v["a"]) == fe_canon(v["b"]))),
                    _r1f(lambda A, B, r, m: int(r["a"] == r["b"])), zero="equal"),
    "Fe2Equal": _fam(["fe2_equal"], 2, False, 1, _bin("fe2"), _out("flag", None),
                     _m1(lambda A, B, v, m: int(fe_canon(v["a"][:5]) == fe_canon(v["b"][:5]) and fe_canon(v["a"][5:]) == fe_canon(v["b"][5:]))),
                     _r1f(lambda A, B, r, m: int(r["a"] == r["b"])), zero="equal2"),
    "PairCanon": _fam(["pair_canon"], 1, True, 2, _un("pf"), _out("pwords", None),
                      _m1(lambda A, B, v, m: (fe_canon(fe_unsign(v["a"][:5], A)), fe_canon(fe_unsign(v["a"][5:], A)))), _r1f(lambda A, B, r, m: r["a"]), zero="pair"),
    # ---- the group law
    "DblPlain": _fam(["dbl<(fq::Mul)0>"], 0, False, 1, XYZ("fe2"), R1_OUT, lambda A, B, v, m: dbl_u(v["X"], v["Y"], v["Z"]), _dbl_ref),
    "DblChain": _fam(["dbl<(fq::Mul)1>"], 0, False, 1, XYZ("fe2"), R1_OUT, lambda A, B, v, m: dbl_u(v["X"], v["Y"], v["Z"]), _dbl_ref),
    "DblSigned": _fam(["dbl<(fq::Mul)2>"], 0, True, 1, XYZ("fe2"), R1_OUT, lambda A, B, v, m: dbl_s(v["X"], v["Y"], v["Z"]), _dbl_ref),
    "AddAffineTable": _fam(["add_affine_table"], 0, True, 1, lambda A, B: R1_IN("fe2", 4) + [("e0", "entry", 1), ("e1", "entry", 1), ("e2", "entry", 1)], R1_OUT,
                           lambda A, B, v, m: add_affine_table(v, m),
                           lambda A, B, r, m: _r1(_ref_add_affine(dict(r, aN=r["e0"], aD=r["e1"], aF=r["e2"]), m, o.f2_mul(r["Ta"], r["Tb"]))), mask=True),
    "AddTable": _fam(["add_table"], 0, False, 1, lambda A, B: R1_IN("fe2", 4) + [("e%d" % c, "entry", 1) for c in range(4)], R1_OUT,
                     lambda A, B, v, m: add_table(v, m),
                     lambda A, B, r, m: _r1(o.ADD((r["X"], r["Y"], r["Z"], r["Ta"], r["Tb"]),
                                                  o.R2neg((r["e0"], r["e1"], r["e2"], r["e3"])) if m else (r["e0"], r["e1"], r["e2"], r["e3"]))), mask=True),
    "PDblPoint": _fam(["pdbl_point"], 0, True, 2, XYZ("pf"), PR1_OUT, lambda A, B, v, m: pdbl_point(v["X"], v["Y"], v["Z"]), _dbl_ref),
    "PAddCore": _fam(["padd_core"], 0, True, 2, lambda A, B: [("pN", "pf", 2), ("pD", "pf", 2), ("pE", "pf", 1), ("pF", "pf", 1), ("qN", "pf", 2), ("qD", "pf", 2), ("qE", "pf", 2), ("qF", "pf", 1)],
                     PR1_OUT, lambda A, B, v, m: padd_core(v),
                     lambda A, B, r, m: _r1(o.ADD_core((r["pN"], r["pD"], r["pE"], r["pF"]), (r["qN"], r["qD"], r["qE"], r["qF"])))),
    "QDblPoint": _fam(["qdbl_point"], 1, True, 4, XYZ("pf"), PR1_T_OUT, lambda A, B, v, m: pdbl_point(v["X"], v["Y"], v["Z"], bool(A)),
                      lambda A, B, r, m: (lambda d: dict(d, T=o.f2_mul(d["Ta"], d["Tb"]) if A else d["Y"]))(_dbl_ref(A, B, r, m))),
    "PAddAffineEntry": _fam(["padd_affine_entry"], 0, True, 2, lambda A, B: R1_IN("pf", 3) + [("aN", "pf", 1), ("aD", "pf", 1), ("aF", "pf", 1)], PR1_OUT,
                            lambda A, B, v, m: padd_affine(v, m, False), lambda A, B, r, m: _r1(_ref_add_affine(r, m, o.f2_mul(r["Ta"], r["Tb"]))), mask=True),
    "QAddAffineEntry": _fam(["qadd_affine_entry"], 0, True, 4, lambda A, B: R1_IN("pf", 3) + [("aN", "pf", 1), ("aD", "pf", 1), ("aF", "pf", 1), ("T", "pf", 1)], PR1_T_OUT,
                            lambda A, B, v, m: padd_affine(v, m, True),
                            lambda A, B, r, m: (lambda d: dict(d, T=o.f2_mul(d["Ta"], d["Tb"])))(_r1(_ref_add_affine(r, m, r["T"]))), mask=True),
}
for _name, _sgn, _leaf in (("Plain", False, "plain"), ("Chain", False, "chain"), ("Signed", True, "signed"), ("Gen", False, "asm")):
    FAMILIES["Fe2Mul" + _name] = _fam(["fe2_mul_" + _leaf], 2, _sgn, 1, _bin("fe2"), _out("fe2", "prod"),
                                      _m1((lambda A, B, v, m: fe2_mul_signed(v["a"], v["b"])) if _sgn else (lambda A, B, v, m: fe2_mul_u(v["a"], v["b"], A))),
                                      _r1f(lambda A, B, r, m: o.f2_mul(r["a"], r["b"])))
    FAMILIES["Fe2Sqr" + _name] = _fam(["fe2_sqr_" + _leaf], 1, _sgn, 1, _un("fe2"), _out("fe2", "prod"),
                                      _m1((lambda A, B, v, m: fe2_sqr_signed(v["a"], A)) if _sgn else (lambda A, B, v, m: fe2_sqr_u(v["a"], A))),
                                      _r1f(lambda A, B, r, m: o.f2_sqr(r["a"])))
MUL_FLAVOURS = ("Plain", "Chain", "Signed", "Gen")        # enum class Mul, in order


def probe_table():
    """[(family, A, B)], the id of an entry its index: FQ_PROBE_TABLE of the probe's source"""
    text = open(PROBE_SRC).read()
    body = text[text.index("#define FQ_PROBE_TABLE(E)"):]
    body = body[:body.index("\n\n")]
    return [(m.group(1), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"\bE\((\w+), (\d+), (\d+)\)", body)]


def entry_name(entry):
    f, A, B = entry
    n = FAMILIES[f]["nargs"]
    return f + ("<%d, %d>" % (A, B) if n == 2 else "<%d>" % A if n == 1 else "")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _intervals(kind, B, signed, finish):
    n = 5 if kind == "fe" else 10
    if kind == "entry":
        signed, B = False, 1
    if kind == "c2" or kind == "pf":
        signed = True
    if finish:                         # what fe_finish / fe_finish_signed hand on: limbs 0, 2, 3, 4 in [0, 2^26), limb 1 up to +-(UNIT - 1)
        five = [(0, M26), (-(UNIT - 1) if signed else 0, UNIT - 1), (0, M26), (0, M26), (0, M26)]
    else:
        five = [(-B * UNIT if signed else 0, B * UNIT)] * 5
    return five * (n // 5)


def zero_class(B, signed, rng, cap=400):
    """(label, delta, limbs): limb vectors within bound B whose value is k p + delta, delta in {0, 1, -1}: k (M, M, M, M, 2^23 - 1)
    limb-wise, the subtraction bias K (M - 7, M, M, M, M), mixtures, each with a carry moved between neighbouring limbs (2^26 out of
    limb i against 1 in limb i + 1, either way; out of limb 4 against 8 in limb 0) and with +-1 on limb 0, as far as every limb stays
    inside the bound"""
    lo, hi = (-B * UNIT if signed else 0), B * UNIT
    pl, bl = [M26] * 4 + [(1 << 23) - 1], [M26 - 7] + [M26] * 4
    ks = list(range(B + 1)) if B <= 9 else sorted({0, 1, 2, B // 2, B - 1, B})
    forms = [("%dp+%dbias" % (k, K), [k * pl[i] + K * bl[i] for i in range(5)]) for k in ks for K in ks if k + K <= B]
    if signed:
        forms += [("-(" + n + ")", [-x for x in f]) for n, f in forms if any(f)]
    moved = []
    for n, f in forms:
        moved.append((n, f))
        for i in range(5):
            for s in (1, -1):
                g = list(f)
                g[i] -= s << 26
                g[(i + 1) % 5] += s * (8 if i == 4 else 1)
                moved.append(("%s carry%+d@%d" % (n, s, i), g))
    out = []
    for n, f in moved:
        for d in (0, 1, -1):
            g = [f[0] + d] + f[1:]
            if all(lo <= x <= hi for x in g):
                assert (value(g) - d) % P == 0
                out.append(("%s %+d" % (n, d), d, g))
    return out if len(out) <= cap else [out[i] for i in sorted(rng.sample(range(len(out)), cap))]


def _equal_pairs(A, B, rng, count):
    """(label, a, b, equal): redundant forms of the residues 0, 1, -1 and of a random residue t, one side off by one in two thirds"""
    za, zb = zero_class(A, False, rng), zero_class(B, False, rng)
    ta, tb = zero_class(A - 1, False, rng), zero_class(B - 1, False, rng)        # bound 0: the all-zero vector alone
    out = []
    for k in range(count):
        if k % 2:
            (na, da, a), (nb, db, b) = rng.choice(za), rng.choice(zb)
        else:
            t = [rng.randint(1, M26 - 1) for _ in range(5)]
            (na, da, a), (nb, db, b) = rng.choice(ta), rng.choice(tb)
            a, b = [x + y for x, y in zip(t, a)], [x + y for x, y in zip(t, b)]
        out.append(("[%s] ? [%s]" % (na, nb), a, b, da == db))
    return out


def vectors(entry):
    """[(pattern, {operand: limbs}, mask)] of an entry; the seed is the entry's name"""
    f, A, B = entry
    fam = FAMILIES[f]
    rng = random.Random(zlib.crc32(entry_name(entry).encode()) + 1)
    ops = fam["operands"](A, B)
    vecs = bd.pattern_vectors({n: _intervals(k, b, fam["signed"], False) for n, k, b in ops}, rng, EXTRA, SAMPLE)
    vecs += [("finish-" + p, v) for p, v in bd.pattern_vectors({n: _intervals(k, b, fam["signed"], True) for n, k, b in ops}, rng, 24, 4)]
    z = fam["zero"]
    if z == "one":
        vecs += [(n, {"a": l}) for n, _, l in zero_class(A, False, rng)]
    elif z == "pair":
        zs = zero_class(A, True, rng)
        vecs += [(n + " | " + n2, {"a": l + l2}) for (n, _, l), (n2, _, l2) in zip(zs, rng.sample(zs, len(zs)))]
    elif z == "equal":
        vecs += [(n, {"a": a, "b": b}) for n, a, b, _ in _equal_pairs(A, B, rng, 300)]
    elif z == "equal2":
        pairs = _equal_pairs(A, B, rng, 600)
        eq, ne = [p for p in pairs if p[3]], [p for p in pairs if not p[3]]
        for case, (res_, ims) in {"re=,im=": (eq, eq), "re=,im!": (eq, ne), "re!,im=": (ne, eq), "re!,im!": (ne, ne)}.items():
            for _ in range(75):
                p, q = rng.choice(res_), rng.choice(ims)
                vecs.append((case + " " + p[0] + " ; " + q[0], {"a": p[1] + q[1], "b": p[2] + q[2]}))
    masks = (0, M32) if fam["mask"] else (0,)
    return [(p, v, m) for m in masks for p, v in vecs]


# ---- records ------------------------------------------------------------------------------------------------------------------------------
def pack(entry, vecs):
    """lane records of an entry's vectors (a list of WORDS-word lists): fam['lanes'] consecutive lanes per vector"""
    f, A, B = entry
    fam = FAMILIES[f]
    ops, lanes = fam["operands"](A, B), fam["lanes"]
    rows = []
    for _, v, mask in vecs:
        for lane in range(lanes):
            row = [0] * WORDS
            k = c = 0
            for name, kind, _ in ops:
                l = v[name]
                if kind == "entry":
                    row[ENTRY_AT + 12 * c:ENTRY_AT + 12 * c + 10] = [x & M32 for x in l]
                    c += 1
                    continue
                if kind == "pf":
                    l = l[5 * (lane & 1):5 * (lane & 1) + 5]
                row[10 * k:10 * k + len(l)] = [x & M32 for x in l]
                k += 1
            row[MASK_AT] = mask
            rows.append(row)
    return rows


def _s32(x):
    return x - (1 << 32) if x >> 31 else x


def unpack(entry, rows):
    """what each vector's lanes stored: a list (one per vector) of lists (one per pair of lanes that holds the element: two for the
    four-lane entries) of {output: limbs as the family reads them, a canonical value or a flag}"""
    f, A, B = entry
    fam = FAMILIES[f]
    lanes, rd = fam["lanes"], (_s32 if fam["signed"] else int)
    res_ = []
    for k in range(len(rows) // lanes):
        views = []
        for p in range(max(1, lanes // 2)):
            r0 = rows[k * lanes + 2 * p]
            r1 = rows[k * lanes + 2 * p + 1] if lanes > 1 else None
            out = {}
            for name, base, kind, promise in fam["outs"](A, B):
                if kind == "flag":
                    out[name] = int(r0[base])
                elif kind == "words":
                    out[name] = sum(int(r0[base + i]) << (32 * i) for i in range(4))
                elif kind == "pwords":
                    out[name] = tuple(sum(int(r[base + i]) << (32 * i) for i in range(4)) for r in (r0, r1))
                elif kind == "pf":
                    rdp = int if promise == "tight" else rd
                    out[name] = [rdp(int(r[base + i])) for r in (r0, r1) for i in range(5)]
                else:
                    rdp = int if promise in ("tight",) or (promise and promise[0] == "ulazy") else rd
                    out[name] = [rdp(int(r0[base + i])) for i in range(5 if kind == "fe" else 10)]
            views.append(out)
        res_.append(views)
    return res_


# ---- the contract -------------------------------------------------------------------------------------------------------------------------
def expected(entry, v, mask):
    f, A, B = entry
    return FAMILIES[f]["ref"](A, B, {n: res(l) for n, l in v.items()}, mask)


def check_outputs(entry, out, want):
    """conditions 1 (residue) and 2 (bound) on one vector's outputs; returns None or what failed"""
    f, A, B = entry
    fam = FAMILIES[f]
    for name, _, kind, promise in fam["outs"](A, B):
        got = out[name]
        if kind in ("flag", "words", "pwords"):
            if got != want[name]:
                return "%s: got %r, the residues give %r" % (name, got, want[name])
            continue
        if res(got) != want[name]:
            return "%s: residue %r, the operation on the input residues gives %r (limbs %r)" % (name, res(got), want[name], got)
        for i, x in enumerate(got):
            if promise == "prod":
                lo, hi = ((-(UNIT - 1) if fam["signed"] else 0), UNIT - 1) if i % 5 == 1 else (0, M26)
            elif promise == "tight":
                lo, hi = 0, UNIT
            else:
                lo, hi = (-promise[1] * UNIT if fam["signed"] and promise[0] == "lazy" else 0), promise[1] * UNIT
            if not lo <= x <= hi:
                return "%s: limb %d = %d outside [%d, %d] (limbs %r)" % (name, i, x, lo, hi, got)
    return None


def model_outputs(entry, v, mask):
    """the model's outputs in the form unpack() gives (element level)"""
    f, A, B = entry
    return FAMILIES[f]["model"](A, B, v, mask)


def limb1_reach(entry, out):
    """largest |limb 1| / UNIT among the product-shaped outputs of one vector (0.0 where there is none)"""
    f, A, B = entry
    m = 0
    for name, _, kind, promise in FAMILIES[f]["outs"](A, B):
        if promise == "prod":
            m = max([m] + [abs(x) for i, x in enumerate(out[name]) if i % 5 == 1])
    return m / UNIT
