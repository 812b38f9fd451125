#!/usr/bin/env python3
"""Interval analysis of the SHIPPED gfx950 bodies (fourq_amd/csrc/ladder_asm_gfx950.inc): the instruction subset of sim.py, run on
integer intervals instead of values, under the operand contracts of CONTRACTS below.  It proves, body by body, that

  * every v_mad_i64_i32 operand lies in [-2^31, 2^31) and every v_mad_u64_u32 operand in [0, 2^32),
  * every 64-bit accumulator stays inside the i64 (signed bodies) or u64 (unsigned bodies) range,
  * no v_lshrrev_b32 / v_lshrrev_b64 operand may be negative,
  * every 32-bit result fits the way its readers interpret it (a value whose interval spans 2^32 or more is unknown),

and it returns the proven interval of every output limb.  CHAINS then checks that each output fits the contract of every body or C++
type it feeds.  fp127.hip.h's static_asserts check the C++ formulas; this checks the instruction streams that run in their place.

Semantics.  A 32-bit register holds a residue mod 2^32; its interval is one integer representative set of it, and a reader may move it by
a multiple of 2^32 to fit its own interpretation (the neg mask 0xFFFFFFFF is -1 to a v_sub_u32).  The limb mask and the neg mask are
concrete: v_and with the mask gives [0, 2^26) (the interval itself when it lies inside one 2^26 block), v_xor / v_xad / v_bitop3 with a neg mask
of 0 or ~0 are exact.  A 64-bit pair written by one instruction keeps its integer interval; v_alignbit(hi, lo, k) of such a pair is
floor(acc / 2^k).  A 64-bit read of a pair whose halves were written separately is allowed only when it is exact (high half 0, low half
in [0, 2^32)).  Anything outside the subset raises.

    python tools/asmgen/bounds.py          # proves every body and every chain edge, prints the proven output intervals and margins
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
INC = os.path.join(ROOT, "fourq_amd", "csrc", "ladder_asm_gfx950.inc")
FP127 = os.path.join(ROOT, "fourq_amd", "csrc", "fp127.hip.h")

UNIT = (1 << 26) + (1 << 15)        # fp127.hip.h: bound of a limb right after normalisation
M26 = (1 << 26) - 1                 # LIMB_MASK
NEG_MASKS = (0, 0xFFFFFFFF)
I32, U32 = (-(1 << 31), (1 << 31) - 1), (0, (1 << 32) - 1)
I64, U64 = (-(1 << 63), (1 << 63) - 1), (0, (1 << 64) - 1)
W32 = 1 << 32


class Finding(Exception):
    """one violated bound: the body, the line of the .inc file, the instruction and what may go wrong"""

    def __init__(self, body, lineno, text, what):
        super().__init__("%s, line %s: %s -- %s" % (body, lineno, text, what))
        self.body, self.lineno, self.text, self.what = body, lineno, text, what


def parse_inc(path=INC):
    """{body name: [(line number, instruction text), ...]} of the include file, read as tests/test_asm_bodies.py::_parse_inc reads it"""
    bodies, cur = {}, None
    with open(path) as fh:
        for n, ln in enumerate(fh, 1):
            m = re.match(r"#define FQ_ASM_(\w+?)(_CLOBBERS)? (.*)$", ln.rstrip("\n"))
            if m and (m.group(2) or m.group(1) == "CLOBBERS"):
                cur = None
            elif m:
                cur = bodies.setdefault(m.group(1), [])
            elif cur is not None:
                t = re.match(r'\s*"(.*?)(?:\\n)?"', ln)
                if t and t.group(1):
                    cur.append((n, t.group(1)))
                if not ln.rstrip().endswith("\\"):
                    cur = None
    return bodies


# ---- intervals ---------------------------------------------------------------------------------------------------------------------
def fit(iv, lo, hi):
    """iv moved by a multiple of 2^32 into [lo, hi], or None when no such move exists (or iv is unknown)"""
    if iv is None or iv[1] - iv[0] > hi - lo:
        return None
    k = -((iv[0] - lo) // W32)                      # smallest shift with iv[0] + k*2^32 >= lo
    a, b = iv[0] + k * W32, iv[1] + k * W32
    return (a, b) if b <= hi else None


def _r32(lo, hi):                                   # a 32-bit result: unknown once it spans 2^32 values
    return (lo, hi) if hi - lo < W32 else None


def _mul(a, b):
    ps = [a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]]
    return (min(ps), max(ps))


def _floordiv(iv, k):
    return (iv[0] >> k, iv[1] >> k)


class Analysis:
    """one pass over a body.  `inputs`: operand ("%N") -> interval; `lines`: [(line number, text)].  After run(): `regs` (the final
    intervals), `findings` (every violated bound, in program order), `margin` (largest |operand| / limit and |accumulator| / limit, with
    where), `trace` (per executed instruction: the intervals of what it wrote, for the soundness test against sim.run)."""

    def __init__(self, name, lines, inputs):
        self.name, self.lines = name, lines
        self.signed = any(t.startswith("v_mad_i64_i32") for _, t in lines)
        self.regs = dict(inputs)
        self.pairs = {}                             # low register -> (interval, token): the 64-bit value of a pair written as one
        self.half = {}                              # register -> (token, 0 low / 1 high)
        self.findings, self.trace = [], []
        self.margin = {"operand": (0.0, None), "accumulator": (0.0, None)}
        self._token, self._where = 0, None

    # ---- bookkeeping ----
    def flag(self, what):
        self.findings.append(Finding(self.name, self._where[0], self._where[1], what))

    def note(self, kind, ratio):
        if ratio > self.margin[kind][0]:
            self.margin[kind] = (ratio, "line %d: %s" % self._where)

    def get(self, op):
        op = op.strip()
        if op in self.regs:
            return self.regs[op]
        if re.fullmatch(r"-?\d+", op):
            v = int(op)
            return (v, v)
        if re.fullmatch(r"0x[0-9a-fA-F]+", op):
            v = int(op, 16)
            return (v, v)
        if re.fullmatch(r"v\d+|%\d+", op):
            raise Finding(self.name, self._where[0], self._where[1], "read of %s before it was written" % op)
        raise ValueError("operand %r" % op)

    def concrete(self, op):
        iv = self.get(op)
        if iv is None or iv[0] != iv[1]:
            return None
        return iv[0] % W32

    def put(self, op, iv):
        op = op.strip()
        self.regs[op] = iv
        self.half.pop(op, None)
        self._wrote.append((op, iv))

    @staticmethod
    def _pair(op):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", op.strip())
        if not m or int(m.group(2)) != int(m.group(1)) + 1 or int(m.group(1)) % 2:
            raise ValueError("64-bit operand %r" % op)
        return "v" + m.group(1), "v" + m.group(2)

    def get64(self, op):
        if op.strip() == "0":
            return (0, 0)
        lo, hi = self._pair(op)
        rec = self.pairs.get(lo)
        if rec is not None and self.half.get(lo) == (rec[1], 0) and self.half.get(hi) == (rec[1], 1):
            return rec[0]
        h, l = self.get(hi), fit(self.get(lo), *U32)
        if h == (0, 0) and l is not None:            # halves written separately: exact only with a zero high half
            return l
        self.flag("64-bit read of %s, whose halves were written separately, is not provably exact" % op)
        return None

    def put64(self, op, iv):
        lo, hi = self._pair(op)
        self._token += 1
        self.pairs[lo] = (iv, self._token)
        if iv is None:
            self.regs[lo] = self.regs[hi] = None
        else:
            k = iv[0] >> 32
            self.regs[lo] = (iv[0] - k * W32, iv[1] - k * W32) if (iv[1] >> 32) == k else None
            self.regs[hi] = _r32(iv[0] >> 32, iv[1] >> 32)
        self.half[lo], self.half[hi] = (self._token, 0), (self._token, 1)
        self._wrote64.append((op.strip(), iv))

    def check64(self, iv, what):
        rng = I64 if self.signed else U64
        if iv is None:
            return None
        if iv[0] < rng[0] or iv[1] > rng[1]:
            self.flag("%s [%d, %d] outside the %s range" % (what, iv[0], iv[1], "i64" if self.signed else "u64"))
            return None
        lim = (1 << 63) if self.signed else (1 << 64)
        self.note("accumulator", max(abs(iv[0]), abs(iv[1])) / lim)
        return iv

    def operand(self, op, signed):
        iv = fit(self.get(op), *(I32 if signed else U32))
        if iv is None:
            self.flag("%s operand %s = %s does not fit %s" % ("v_mad_i64_i32" if signed else "v_mad_u64_u32", op, _fmt(self.get(op)),
                                                                "[-2^31, 2^31)" if signed else "[0, 2^32)"))
        else:
            self.note("operand", max(abs(iv[0]), abs(iv[1])) / ((1 << 31) if signed else (1 << 32)))
        return iv

    # ---- the instruction subset of sim.py ----
    def run(self):
        for lineno, ln in self.lines:
            ln = ln.strip()
            if not ln or ln.startswith("."):
                continue
            self._where, self._wrote, self._wrote64 = (lineno, ln), [], []
            self.step(ln)
            self.trace.append((lineno, ln, self._wrote, self._wrote64))
        return self

    def step(self, ln):
        mn, rest = ln.split(None, 1)
        extra = None
        if " bitop3:" in rest:
            rest, extra = rest.split(" bitop3:")
        ops = [o.strip() for o in rest.split(",")]
        base = re.sub(r"_e(32|64)$", "", mn)
        g = self.get
        if base == "v_mov_b32":
            self.put(ops[0], g(ops[1]))
        elif base in ("v_add_u32", "v_sub_u32"):
            a, b = g(ops[1]), g(ops[2])
            if a is None or b is None:
                self.put(ops[0], None)
            elif base == "v_add_u32":
                self.put(ops[0], _r32(a[0] + b[0], a[1] + b[1]))
            else:
                self.put(ops[0], _r32(a[0] - b[1], a[1] - b[0]))
        elif base == "v_lshlrev_b32":
            k, a = self.concrete(ops[1]), g(ops[2])
            self.put(ops[0], None if a is None else _r32(a[0] << k, a[1] << k))
        elif base == "v_lshrrev_b32":
            k, a = self.concrete(ops[1]), g(ops[2])
            if a is None or a[0] < 0 or a[1] >= W32:
                self.flag("v_lshrrev_b32 operand %s = %s may be negative or does not fit [0, 2^32)" % (ops[2], _fmt(a)))
                self.put(ops[0], None)
            else:
                self.put(ops[0], _floordiv(a, k))
        elif base == "v_lshl_add_u32":
            a, k, c = g(ops[1]), self.concrete(ops[2]), g(ops[3])
            self.put(ops[0], None if a is None or c is None else _r32((a[0] << k) + c[0], (a[1] << k) + c[1]))
        elif base == "v_and_b32":
            m, x = self.concrete(ops[1]), ops[2]
            if m is None:
                m, x = self.concrete(ops[2]), ops[1]
            a = g(x)
            if m == M26:
                if a is not None and a[0] >> 26 == a[1] >> 26:
                    k = (a[0] >> 26) << 26
                    self.put(ops[0], (a[0] - k, a[1] - k))
                else:
                    self.put(ops[0], (0, M26))
            elif m == 0:
                self.put(ops[0], (0, 0))
            else:
                raise ValueError("v_and_b32 with an operand that is neither the limb mask nor 0: %r" % ln)
        elif base == "v_xor_b32":
            m, x = self.concrete(ops[1]), ops[2]
            if m not in NEG_MASKS:
                m, x = self.concrete(ops[2]), ops[1]
            a = g(x)
            if m == 0:
                self.put(ops[0], a)
            elif m == 0xFFFFFFFF:
                self.put(ops[0], None if a is None else (-a[1] - 1, -a[0] - 1))      # ~x == -x - 1 (mod 2^32)
            else:
                raise ValueError("v_xor_b32 without a concrete neg mask: %r" % ln)
        elif base == "v_xad_u32":                   # (x ^ neg mask) + c: the exact v_xor_b32 above, then v_add_u32
            m, a, c = self.concrete(ops[2]), g(ops[1]), g(ops[3])
            if m not in NEG_MASKS:
                raise ValueError("v_xad_u32 without a concrete neg mask: %r" % ln)
            if m and a is not None:
                a = (-a[1] - 1, -a[0] - 1)
            self.put(ops[0], None if a is None or c is None else _r32(a[0] + c[0], a[1] + c[1]))
        elif base == "v_bitop3_b32":
            if int(extra, 16) != 0xCA:
                raise ValueError("bitop3 table " + extra)
            m = self.concrete(ops[1])
            if m not in NEG_MASKS:
                raise ValueError("v_bitop3_b32 without a concrete neg mask: %r" % ln)
            self.put(ops[0], g(ops[2]) if m else g(ops[3]))
        elif base == "v_alignbit_b32":
            k = self.concrete(ops[3])
            hi, lo = ops[1], ops[2]
            ph, pl = self.half.get(hi), self.half.get(lo)
            m = re.fullmatch(r"v(\d+)", lo)
            if ph is None or pl is None or ph != (pl[0], 1) or pl[1] != 0 or not m or "v%d" % (int(m.group(1)) + 1) != hi:
                raise ValueError("v_alignbit_b32 of two registers that are not one accumulator pair: %r" % ln)
            acc = self.pairs[lo][0]
            self.put(ops[0], None if acc is None else _r32(*_floordiv(acc, k)))    # bits k..k+31 of the pair == floor(acc / 2^k) mod 2^32
        elif base in ("v_mad_i64_i32", "v_mad_u64_u32"):
            if ops[1] != "vcc":
                raise ValueError("carry-out operand " + ops[1])
            signed = base == "v_mad_i64_i32"
            if signed != self.signed:
                raise ValueError("a body that mixes signed and unsigned multiply-adds: %r" % ln)
            a, b = self.operand(ops[2], signed), self.operand(ops[3], signed)
            c = self.get64(ops[4])
            if a is None or b is None or c is None:
                self.put64(ops[0], None)
            else:
                p = _mul(a, b)
                self.put64(ops[0], self.check64((p[0] + c[0], p[1] + c[1]), "accumulator"))
        elif base == "v_ashrrev_i64":
            k, a = self.concrete(ops[1]), self.get64(ops[2])
            if a is not None and (a[0] < I64[0] or a[1] > I64[1]):     # an unsigned body's accumulator of 2^63 or more reads as negative
                self.flag("v_ashrrev_i64 operand %s = %s does not fit the i64 range" % (ops[2], _fmt(a)))
                a = None
            self.put64(ops[0], None if a is None else _floordiv(a, k))
        elif base == "v_lshrrev_b64":
            k, a = self.concrete(ops[1]), self.get64(ops[2])
            if a is None or a[0] < 0:
                self.flag("v_lshrrev_b64 operand %s = %s may be negative" % (ops[2], _fmt(a)))
                self.put64(ops[0], None)
            else:
                self.put64(ops[0], _floordiv(a, k))
        elif base == "v_lshl_add_u64":
            s, k, c = self.get64(ops[1]), self.concrete(ops[2]), self.get64(ops[3])
            if s is None or c is None:
                self.put64(ops[0], None)
            else:
                self.put64(ops[0], self.check64(((s[0] << k) + c[0], (s[1] << k) + c[1]), "v_lshl_add_u64 result"))
        else:
            raise ValueError("instruction %r is outside the analysed subset" % ln)


def _fmt(iv):
    return "unknown" if iv is None else "[%d, %d]" % iv


# ---- the contract table ----------------------------------------------------------------------------------------------------------------
# Limb intervals of the C++ types at the call sites (ladder_asm.hip.h, kernels.hip.h, curve.hip.h).  A limb interval is an integer range;
# a body's register holds it mod 2^32.
def signed(B):
    """Fe2<B> of the signed flavour (ladder phase, table bodies): |limb| <= B * UNIT"""
    return [(-B * UNIT, B * UNIT)] * 10


def unsigned(B):
    """Fe2<B> of the unsigned flavour: limb in [0, B * UNIT]"""
    return [(0, B * UNIT)] * 10


TIGHT = unsigned(1)                 # a table entry, EntryRegs, fe_carry / fe_unsign output: non-negative, limb <= UNIT
UNPACK = ([(0, M26)] * 4 + [(0, (1 << 24) - 1)]) * 2        # fe_unpack of any 128-bit word: limbs 0-3 in [0, 2^26), limb 4 in [0, 2^24)


def bias_limb(k, i):                # fp127.hip.h: limbs of k * (2^130 - 8)
    return k * (M26 - 7 if i == 0 else M26)


def cols_ok(weighted):              # fp127.hip.h, restated (tests/test_asm_bounds.py checks the header's text)
    return weighted * 5 * 8 <= ((2 ** 64 - 1 - (1 << 41)) // (UNIT * UNIT))


def mulu_admitted():
    """every (A, B) that fe2_mul_asm's static_asserts admit, with the conditions of the helpers it calls (fe_neg of a.im: bias large
    enough; every limb of a and of -a.im a 32-bit value)"""
    out = []
    for A in range(1, 64):
        for B in range(1, 64):
            if (cols_ok((2 * A + 1) * B) and 8 * B * UNIT < (1 << 32) and (A + 1) * (M26 - 7) >= A * UNIT
                    and (A + 1) * M26 < (1 << 32) and A * UNIT < (1 << 32)):
                out.append((A, B))
    return out


def sqru_admitted():
    """every A that fe2_sqr_asm's static_asserts admit (and fe_add / fe_sub / fe_dbl of its operands: limbs below 2^32)"""
    return [A for A in range(1, 64) if cols_ok((2 * A + 1) * (2 * A)) and 8 * (2 * A) * UNIT < (1 << 32) and (2 * A + 1) * UNIT < (1 << 32)]


def mulu_inputs(A, B):
    """fe2_mul_asm<A, B>: a (ten limbs in [0, A*UNIT]), na = fe_neg(a.im) = bias(A+1) - a.im, b (ten limbs in [0, B*UNIT])"""
    na = [(bias_limb(A + 1, i) - A * UNIT, bias_limb(A + 1, i)) for i in range(5)]
    return unsigned(A) + na + unsigned(B)


def sqru_inputs(A):
    """fe2_sqr_asm<A>: d = fe_sub(a.re, a.im) = a.re + bias(A+1) - a.im, s = a.re + a.im, t = 2 a.re, a.im"""
    d = [(bias_limb(A + 1, i) - A * UNIT, A * UNIT + bias_limb(A + 1, i)) for i in range(5)]
    return d + [(0, 2 * A * UNIT)] * 5 + [(0, 2 * A * UNIT)] * 5 + [(0, A * UNIT)] * 5


# Per body: operands in asm order as (name, first operand, limb intervals or a u32 value, role).  role "in" / "io": what the body may
# assume (the input contract); "io" / "out": what it must deliver (the output contract, the C++ type the operand has at the call site).
# "mask" is LIMB_MASK, "neg" the neg mask (every body that takes one is analysed once per value).
def _fe2(name, base, ins=None, out=None):
    return (name, base, ins, out)


CONTRACTS = {
    # ladder_asm.hip.h: dbl_asm(Fe2<1>& X, Y, Z)
    "DBL": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)), ("mask", 30)],
    # dblt_asm(Fe2<1>& X, Y, Z, Fe2<1>& T)
    "DBLT": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)),
             _fe2("T", 30, None, signed(1)), ("mask", 40)],
    # add_asm(R1& q, const Fe2<1>& T, const EntryRegs& t, u32 neg_mask): q.X, q.Y, q.Z Fe2<1>, q.Ta Fe2<4>, q.Tb Fe2<2> (curve.hip.h R1)
    "ADD": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)),
            _fe2("Ta", 30, None, signed(4)), _fe2("Tb", 40, None, signed(2)), _fe2("T", 50, signed(1)),
            _fe2("N", 60, TIGHT), _fe2("D", 70, TIGHT), _fe2("E", 80, TIGHT), _fe2("F", 90, TIGHT), ("neg", 100), ("mask", 101)],
    # step_asm(R1& q, const EntryRegs& t, u32 neg_mask)
    "STEP": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)),
             _fe2("Ta", 30, None, signed(4)), _fe2("Tb", 40, None, signed(2)),
             _fe2("N", 50, TIGHT), _fe2("D", 60, TIGHT), _fe2("E", 70, TIGHT), _fe2("F", 80, TIGHT), ("neg", 90), ("mask", 91)],
    # tau_asm / upsilon_asm / chi_asm(Fe2<1>& X, Y, Z)
    "TAU": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)), ("mask", 30)],
    "UPSILON": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)), ("mask", 30)],
    "CHI": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)), ("mask", 30)],
    # taudual_asm(Fe2<1>& X, Y, Z, Fe2<2>& N3, Fe2<2>& D3, Fe2<1>& F3)
    "TAUDUAL": [_fe2("X", 0, signed(1), signed(1)), _fe2("Y", 10, signed(1), signed(1)), _fe2("Z", 20, signed(1), signed(1)),
                _fe2("N3", 30, None, signed(2)), _fe2("D3", 40, None, signed(2)), _fe2("F3", 50, None, signed(1)), ("mask", 60)],
    # r1_to_r2_asm(const R1& p) -> R2 (tight): p.X, p.Y, p.Z Fe2<1>, p.Ta Fe2<4>, p.Tb Fe2<2>
    "R1TOR2": [_fe2("N", 0, None, TIGHT), _fe2("D", 10, None, TIGHT), _fe2("E", 20, None, TIGHT), _fe2("F", 30, None, TIGHT),
               _fe2("X", 40, signed(1)), _fe2("Y", 50, signed(1)), _fe2("Z", 60, signed(1)), _fe2("Ta", 70, signed(4)), _fe2("Tb", 80, signed(2)),
               ("mask", 90)],
    # table_add_asm(R2& q, const Fe2<2>& N3, const Fe2<2>& D3, const Fe2<1>& E3, const Fe2<1>& F3)
    "TABLEADD": [_fe2("qN", 0, TIGHT, TIGHT), _fe2("qD", 10, TIGHT, TIGHT), _fe2("qE", 20, TIGHT, TIGHT), _fe2("qF", 30, TIGHT, TIGHT),
                 _fe2("N3", 40, signed(2)), _fe2("D3", 50, signed(2)), _fe2("E3", 60, signed(1)), _fe2("F3", 70, signed(1)), ("mask", 80)],
}
for _A, _B in mulu_admitted():      # fe2_mul_asm<A, B> -> Fe2<1> of the unsigned flavour
    _ins = mulu_inputs(_A, _B)
    CONTRACTS["MULU<%d,%d>" % (_A, _B)] = [_fe2("C", 0, None, TIGHT), _fe2("A", 10, _ins[:10]), ("na", 20, _ins[10:15]), _fe2("B", 25, _ins[15:]),
                                           ("mask", 35)]
for _A in sqru_admitted():          # fe2_sqr_asm<A> -> Fe2<1> of the unsigned flavour
    _ins = sqru_inputs(_A)
    CONTRACTS["SQRU<%d>" % _A] = [_fe2("C", 0, None, TIGHT), ("d", 10, _ins[:5]), ("s", 15, _ins[5:10]), ("t", 20, _ins[10:15]),
                                  ("im", 25, _ins[15:]), ("mask", 30)]


def body_of(contract_name):
    return contract_name.split("<")[0]


def operands(contract_name):
    """{name: (first operand, limb count, input intervals or None, output intervals or None)}; u32 operands have limb count 1"""
    out = {}
    for op in CONTRACTS[contract_name]:
        if len(op) == 2:
            out[op[0]] = (op[1], 1, None, None)
        elif len(op) == 3:                            # a bare GF(p) operand of MULU / SQRU
            out[op[0]] = (op[1], 5, op[2], None)
        else:
            out[op[0]] = (op[1], 10, op[2], op[3])
    return out


def input_regs(contract_name, neg=0, override=None):
    """operand register -> interval under the contract (override: {operand name: limb intervals} replaces entries)"""
    regs = {}
    for name, (base, n, ins, _) in operands(contract_name).items():
        if override and name in override:
            ins = override[name]
        if name == "mask":
            regs["%%%d" % base] = (M26, M26)
        elif name == "neg":
            regs["%%%d" % base] = (neg, neg)
        elif ins is not None:
            for i in range(n):
                regs["%%%d" % (base + i)] = ins[i]
    return regs


def neg_values(contract_name):
    return NEG_MASKS if "neg" in operands(contract_name) else (0,)


_BODIES = None


def shipped():
    global _BODIES
    if _BODIES is None:
        _BODIES = parse_inc()
    return _BODIES


def analyse(contract_name, neg=0, lines=None, override=None):
    """run the analysis of one body under its contract; returns the Analysis (findings empty = proven)"""
    body = body_of(contract_name)
    return Analysis(contract_name if neg == 0 else contract_name + " neg=~0", lines or shipped()[body],
                    input_regs(contract_name, neg, override)).run()


def proven_outputs(contract_name, lines=None, override=None):
    """{output operand: ten limb intervals}, the hull over the neg-mask values, each interval in the representation of the operand's
    C++ type (signed limbs for the signed flavour, non-negative otherwise); raises the first finding if the body is not proven"""
    res = {}
    for neg in neg_values(contract_name):
        a = analyse(contract_name, neg, lines, override)
        if a.findings:
            raise a.findings[0]
        for name, (base, n, _, out) in operands(contract_name).items():
            if out is None:
                continue
            ivs = []
            for i in range(n):
                iv = a.regs.get("%%%d" % (base + i))
                rep = fit(iv, out[i][0], out[i][0] + W32 - 1)
                if rep is None:
                    raise Finding(contract_name, "-", "output %s limb %d" % (name, i), "unknown value %s" % _fmt(iv))
                ivs.append(rep)
            prev = res.get(name)
            res[name] = ivs if prev is None else [(min(p[0], q[0]), max(p[1], q[1])) for p, q in zip(prev, ivs)]
    return res


def within(ivs, contract):
    """every limb interval inside the contract's (after a move by a multiple of 2^32): the limbs that are not"""
    return [i for i, (iv, c) in enumerate(zip(ivs, contract)) if fit(iv, c[0], c[1]) is None]


# ---- the chain: every edge where one body's output feeds another body or a C++ value of a given type ---------------------------------
# (producer, output operand) -> (consumer, input operand), or a C++ consumer given by its limb intervals.  kernels.hip.h, ladder_endo_nibbles_by and
# its kin ("the ladders"): start_table -> DBLT / DBL, DBLT -> ADD, ADD -> DBLT / DBL, DBL -> DBL / DBLT, the result -> r1_unsign /
# store_r1_signed (fe_unsign / fe_unsign_wide of Fe2<1>, Ta Fe2<4>, Tb Fe2<2>).  build_table_endo_lds_asm: R1TOR2 -> table,
# TAU -> UPSILON / CHI (and parked in LDS as Fe2<1>), UPSILON / CHI -> TAUDUAL, TAUDUAL -> TAU (next step) and -> TABLEADD, TABLEADD ->
# table -> TABLEADD / ADD / STEP.  Sources: fe_unpack of any input word, start_table's fe2_carry (bound-1 non-negative), table entries.
def _cpp(name, ivs):
    return ("C++ " + name, ivs)


SOURCES = {                          # values that enter a body from C++: (description, limb intervals)
    "fe_unpack": UNPACK,             # every coordinate the ABI hands in ([0, 2^128) accepted)
    "start_table": TIGHT,            # fe2_carry(N - D), fe2_carry(D + N), the entry's E (curve.hip.h start_table)
    "entry": TIGHT,                  # a table entry / EntryRegs (tight non-negative; fe_unpack'd table words are inside it)
}

CHAINS = [
    # the ladders
    (("start_table", None), ("DBLT", "X")), (("start_table", None), ("DBLT", "Y")), (("start_table", None), ("DBLT", "Z")),
    (("start_table", None), ("DBL", "X")), (("start_table", None), ("DBL", "Y")), (("start_table", None), ("DBL", "Z")),
    (("DBLT", "X"), ("ADD", "X")), (("DBLT", "Y"), ("ADD", "Y")), (("DBLT", "Z"), ("ADD", "Z")), (("DBLT", "T"), ("ADD", "T")),
    (("ADD", "X"), ("DBLT", "X")), (("ADD", "Y"), ("DBLT", "Y")), (("ADD", "Z"), ("DBLT", "Z")),
    (("ADD", "X"), ("DBL", "X")), (("ADD", "Y"), ("DBL", "Y")), (("ADD", "Z"), ("DBL", "Z")),
    (("DBL", "X"), ("DBL", "X")), (("DBL", "Y"), ("DBL", "Y")), (("DBL", "Z"), ("DBL", "Z")),
    (("DBL", "X"), ("DBLT", "X")), (("DBL", "Y"), ("DBLT", "Y")), (("DBL", "Z"), ("DBLT", "Z")),
    (("STEP", "X"), ("STEP", "X")), (("STEP", "Y"), ("STEP", "Y")), (("STEP", "Z"), ("STEP", "Z")),
    (("start_table", None), ("STEP", "X")), (("start_table", None), ("STEP", "Y")), (("start_table", None), ("STEP", "Z")),
    (("entry", None), ("ADD", "N")), (("entry", None), ("ADD", "D")), (("entry", None), ("ADD", "E")), (("entry", None), ("ADD", "F")),
    (("entry", None), ("STEP", "N")), (("entry", None), ("STEP", "D")), (("entry", None), ("STEP", "E")), (("entry", None), ("STEP", "F")),
    (("fe_unpack", None), ("ADD", "N")), (("fe_unpack", None), ("ADD", "E")),                          # *_fixed: the caller's table words
    (("ADD", "X"), _cpp("fe_unsign<1> (r1_unsign / store_r1_signed)", signed(1))),
    (("ADD", "Y"), _cpp("fe_unsign<1> (r1_unsign / store_r1_signed)", signed(1))),
    (("ADD", "Z"), _cpp("fe_unsign<1> (r1_unsign / store_r1_signed)", signed(1))),
    (("ADD", "Ta"), _cpp("R1::Ta Fe2<4> -> fe_unsign<4>", signed(4))), (("ADD", "Tb"), _cpp("R1::Tb Fe2<2> -> fe_unsign<2>", signed(2))),
    (("STEP", "Ta"), _cpp("R1::Ta Fe2<4>", signed(4))), (("STEP", "Tb"), _cpp("R1::Tb Fe2<2>", signed(2))),
    # the table phase
    (("fe_unpack", None), ("R1TOR2", "X")), (("fe_unpack", None), ("R1TOR2", "Y")), (("fe_unpack", None), ("R1TOR2", "Z")),
    (("fe_unpack", None), ("R1TOR2", "Ta")), (("fe_unpack", None), ("R1TOR2", "Tb")),
    (("fe_unpack", None), ("TAU", "X")), (("fe_unpack", None), ("TAU", "Y")), (("fe_unpack", None), ("TAU", "Z")),
    (("R1TOR2", "N"), ("TABLEADD", "qN")), (("R1TOR2", "D"), ("TABLEADD", "qD")), (("R1TOR2", "E"), ("TABLEADD", "qE")),
    (("R1TOR2", "F"), ("TABLEADD", "qF")),
    (("R1TOR2", "N"), _cpp("table entry (ADD / STEP / start_table / scans)", TIGHT)),
    (("TAU", "X"), ("UPSILON", "X")), (("TAU", "Y"), ("UPSILON", "Y")), (("TAU", "Z"), ("UPSILON", "Z")),
    (("TAU", "X"), ("CHI", "X")), (("TAU", "Y"), ("CHI", "Y")), (("TAU", "Z"), ("CHI", "Z")),
    (("TAU", "X"), _cpp("park_xyz Fe2<1>", signed(1))),
    (("UPSILON", "X"), ("TAUDUAL", "X")), (("UPSILON", "Y"), ("TAUDUAL", "Y")), (("UPSILON", "Z"), ("TAUDUAL", "Z")),
    (("CHI", "X"), ("TAUDUAL", "X")), (("CHI", "Y"), ("TAUDUAL", "Y")), (("CHI", "Z"), ("TAUDUAL", "Z")),
    (("TAUDUAL", "X"), ("TAU", "X")), (("TAUDUAL", "Y"), ("TAU", "Y")), (("TAUDUAL", "Z"), ("TAU", "Z")),
    (("TAUDUAL", "N3"), ("TABLEADD", "N3")), (("TAUDUAL", "D3"), ("TABLEADD", "D3")), (("TAUDUAL", "Z"), ("TABLEADD", "E3")),
    (("TAUDUAL", "F3"), ("TABLEADD", "F3")),
    (("TABLEADD", "qN"), ("TABLEADD", "qN")), (("TABLEADD", "qD"), ("TABLEADD", "qD")), (("TABLEADD", "qE"), ("TABLEADD", "qE")),
    (("TABLEADD", "qF"), ("TABLEADD", "qF")),
    (("TABLEADD", "qN"), ("ADD", "N")), (("TABLEADD", "qD"), ("ADD", "D")), (("TABLEADD", "qE"), ("ADD", "E")), (("TABLEADD", "qF"), ("ADD", "F")),
    (("R1TOR2", "N"), ("ADD", "N")), (("R1TOR2", "F"), ("ADD", "F")),
    # the unsigned products: an output of bound 1 feeds every product again (fe2_mul_asm<1, 1>, fe2_sqr_asm<1>)
    (("MULU<1,1>", "C"), ("MULU<1,1>", "A")), (("MULU<1,1>", "C"), ("MULU<1,1>", "B")), (("SQRU<1>", "C"), ("MULU<1,1>", "A")),
    (("MULU<1,1>", "C"), _cpp("Fe2<1> of the unsigned flavour", unsigned(1))),
    (("SQRU<1>", "C"), _cpp("Fe2<1> of the unsigned flavour", unsigned(1))),
    (("fe_unpack", None), ("MULU<1,1>", "A")), (("fe_unpack", None), ("MULU<1,1>", "B")),
]


def check_chains(outputs):
    """outputs: {contract name: proven_outputs(...)}.  Returns [(edge, limbs that do not fit)] for every edge that does not close."""
    bad = []
    for (src, sname), dst in CHAINS:
        ivs = SOURCES[src] if sname is None else outputs[src][sname]
        if isinstance(dst[1], list):
            want = dst[1]
        else:
            want = operands(dst[0])[dst[1]][2]
        miss = within(ivs, want)
        if miss:
            bad.append((((src, sname), dst[0] if isinstance(dst[1], list) else dst), miss))
    return bad


def prove_all():
    """every contract: (proven outputs, margins per neg value).  Raises the first finding of a body that is not proven."""
    outs, margins = {}, {}
    for name in CONTRACTS:
        outs[name] = proven_outputs(name)
        margins[name] = [analyse(name, neg).margin for neg in neg_values(name)]
    return outs, margins


def report(outs, margins):
    lines = []
    worst = (0.0, None)
    for name in CONTRACTS:
        if name.startswith(("MULU<", "SQRU<")) and name not in ("MULU<1,1>", "SQRU<1>"):
            continue
        for m in margins[name]:
            for kind, (r, where) in m.items():
                if r > worst[0]:
                    worst = (r, "%s %s (%s)" % (name, kind, where))
        parts = []
        for op, ivs in outs[name].items():
            lo, hi = min(iv[0] for iv in ivs), max(iv[1] for iv in ivs)
            parts.append("%s limbs in [%s, %s]" % (op, _units(lo), _units(hi)))
        opr = max(m["operand"][0] for m in margins[name])
        acc = max(m["accumulator"][0] for m in margins[name])
        lines.append("%-10s %s; largest operand %.3f of its limit, accumulator %.2e" % (name, "; ".join(parts), opr, acc))
    for name in CONTRACTS:                              # the smallest margin over every admitted MULU / SQRU instance too
        for m in margins[name]:
            for kind, (r, where) in m.items():
                if r > worst[0]:
                    worst = (r, "%s %s (%s)" % (name, kind, where))
    lines.append("smallest margin: %.4f of the limit, %s" % worst)
    return "\n".join(lines)


def _units(x):
    if x == 0:
        return "0"
    return "%s%.6f UNIT" % ("-" if x < 0 else "", abs(x) / UNIT)


# ---- corner inputs (tests/test_asm_bounds.py, tests/test_gpu_asm_corners.py) ----------------------------------------------------------
def _component(ivs, pattern, rng):
    """five limbs inside `ivs` by pattern: every limb at its max / min, alternating, random extremes, a top limb in [2^23, 2^24), random"""
    out = []
    for i, (lo, hi) in enumerate(ivs):
        if pattern == "max" or (pattern == "alt" and i % 2 == 0) or (pattern == "alt2" and i % 2):
            out.append(hi)
        elif pattern in ("min", "alt", "alt2"):
            out.append(lo)
        elif pattern == "ext":
            out.append(rng.choice((lo, hi)))
        elif pattern == "top" and i == 4 and lo <= (1 << 23) and hi >= (1 << 24) - 1:
            out.append(rng.randrange(1 << 23, 1 << 24))
        elif pattern == "top":
            out.append(rng.choice((lo, hi, rng.randint(lo, hi))))
        else:
            out.append(rng.randint(lo, hi))
    return out


def _free(contract_name):
    """the independent inputs of a contract: {name: ten limb intervals}.  MULU's -a.im and SQRU's d, s, t follow from them."""
    body = body_of(contract_name)
    if body == "MULU":
        A, B = map(int, contract_name[5:-1].split(","))
        return {"A": unsigned(A), "B": unsigned(B)}
    if body == "SQRU":
        return {"a": unsigned(int(contract_name[5:-1]))}
    return {name: ins for name, (_, n, ins, _) in operands(contract_name).items() if ins is not None and n == 10}


def corner_vectors(contract_name, rng, count):
    """`count` input vectors at the corners of a contract, {operand: limbs as integers}: all limbs at their max, at their min, the two
    alternating patterns, every component (re / im of an operand) at its max or its min in every combination -- for bodies with more
    than count / 2 such combinations (ADD, STEP, R1TOR2, TABLEADD) a random sample of count / 2 of them, so there only all-max and
    all-min are certain -- then random extremes, top limbs in [2^23, 2^24) and random limbs"""
    free = _free(contract_name)
    comps = [(name, h) for name in free for h in (0, 1)]
    pats = []
    for p in ("max", "min", "alt", "alt2"):
        pats.append({c: p for c in comps})
    n = len(comps)
    combos = range(1 << n) if (1 << n) <= count // 2 else rng.sample(range(1 << n), count // 2)
    for bits in combos:
        pats.append({c: ("max" if bits >> k & 1 else "min") for k, c in enumerate(comps)})
    while len(pats) < count:
        pats.append({c: rng.choice(("ext", "ext", "top", "rand")) for c in comps})
    vecs = []
    for pat in pats[:count]:
        v = {name: _component(free[name][:5], pat[(name, 0)], rng) + _component(free[name][5:], pat[(name, 1)], rng) for name in free}
        body = body_of(contract_name)
        if body == "MULU":
            A = int(contract_name[5:-1].split(",")[0])
            v["na"] = [bias_limb(A + 1, i) - v["A"][5 + i] for i in range(5)]
        elif body == "SQRU":
            A = int(contract_name[5:-1])
            re_, im = v["a"][:5], v["a"][5:]
            v["d"] = [re_[i] + bias_limb(A + 1, i) - im[i] for i in range(5)]
            v["s"] = [re_[i] + im[i] for i in range(5)]
            v["t"] = [2 * re_[i] for i in range(5)]
            v["im"] = im
        vecs.append(v)
    return vecs


def pattern_vectors(free, rng, extra, sample=64):
    """corner inputs for operands that are no contract of a generated body (tests/field_model.py): `free` maps an operand to its limb
    intervals, a multiple of five of them, and every five are a component.  (pattern, {operand: limbs}) for: all components at max, at
    min, the two alternating patterns; every combination of components at max / min (a seeded sample of `sample` when there are more
    than that); then `extra` vectors of random extremes, top limbs and random limbs per component.  corner_vectors is not built on
    this: its vectors seed the existing tests and stay as they are."""
    comps = [(name, h) for name in free for h in range(len(free[name]) // 5)]
    pats = [(p, {c: p for c in comps}) for p in ("max", "min", "alt", "alt2")]
    n = len(comps)
    combos = range(1 << n) if (1 << n) <= sample else rng.sample(range(1 << n), sample)
    for bits in combos:
        pats.append(("combo%x" % bits, {c: ("max" if bits >> k & 1 else "min") for k, c in enumerate(comps)}))
    for _ in range(extra):
        pats.append(("mixed", {c: rng.choice(("ext", "ext", "top", "rand")) for c in comps}))
    return [(label, {name: [x for h in range(len(free[name]) // 5) for x in _component(free[name][5 * h:5 * h + 5], pat[(name, h)], rng)]
                     for name in free}) for label, pat in pats]


def registers(contract_name, vec, neg=0):
    """sim.py registers of an input vector (limbs mod 2^32), the limb mask and the neg mask included"""
    regs = {}
    for name, (base, n, _, _) in operands(contract_name).items():
        if name == "mask":
            regs["%%%d" % base] = M26
        elif name == "neg":
            regs["%%%d" % base] = neg
        elif name in vec:
            for i in range(n):
                regs["%%%d" % (base + i)] = vec[name][i] % W32
    return regs


def main():
    outs, margins = prove_all()
    bad = check_chains(outs)
    print(report(outs, margins))
    print("%d contracts proven (%d MULU, %d SQRU instances), %d chain edges, %d open" % (
        len(CONTRACTS), len(mulu_admitted()), len(sqru_admitted()), len(CHAINS), len(bad)))
    for edge, miss in bad:
        print("open edge", edge, "limbs", miss)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
