"""Points and 32-byte strings built to reach the states of the device's wire-format code (curve.hip.h: point_decode, point_encode,
fe2_sign) that random strings and valid keys [m]G do not: a half of x that is 0, an intermediate value of decode that is 0 modulo p
without being the integer 0, y in a subfield, y words on the limb boundaries of fe_unpack, the refused encodings, and points outside
the subgroup of order N.  Pure Python, deterministic; shared by the CPU tests (test_adversarial_points.py, which proves that every
family has the property it is for), the fixture generator (golden/make_adversarial_points.py) and the GPU tests
(test_gpu_adversarial_points.py).  A point family is a list of (label, (x, y)); a string family a list of (label, 32 bytes).  The square
root in GF(p^2) and the double-and-add below are written from the mathematics: p = 3 (mod 4), so a root in GF(p) is a^((p+1)/4)."""
import functools
import random

import curve4q_oracle as o

P = o.P127
N = o.N
HALF = 1 << 126                           # bit 126, the sign bit of a coordinate; also 1/2 modulo p
ORDER = 392 * N                           # the order of the whole group
NEUTRAL = ((0, 0), (1, 0))
E_X = (1, 2, HALF - 1, HALF, HALF + 1, P - 2, P - 1)
# the limb boundaries of fe_unpack (26-bit limbs from bit 0, the top limb from bit 104) and the sign and fold boundaries
E_Y = (0, 1, 2, (1 << 26) - 1, 1 << 26, (1 << 52) - 1, 1 << 52, 1 << 78, (1 << 104) - 1, 1 << 104, HALF - 1, HALF, P - 2, P - 1)


def word_name(v):
    for base, name in ((P, "p"), (HALF, "2^126")):
        if abs(v - base) <= 2:
            return name + ("" if v == base else "%+d" % (v - base))
    if v > 2 and (v & (v - 1)) == 0:
        return "2^%d" % (v.bit_length() - 1)
    if v > 2 and (v & (v + 1)) == 0:
        return "2^%d-1" % v.bit_length()
    return "%d" % v


# ---- square roots ---------------------------------------------------------------------------------------------------------------
def fp_sqrt(a):
    r = pow(a % P, 1 << 125, P)           # (p + 1) / 4 = 2^125
    return r if r * r % P == a % P else None


def f2_sqrt(a):
    """a root of a in GF(p^2), or None.  a1 = 0: -1 is no square in GF(p), so one of a0, -a0 has a root r there; the root of a is r or
    r i.  Otherwise a root (r, i) has r^2 - i^2 = a0 and 2 r i = a1, so r^2 = (a0 +- n) / 2 with n^2 = a0^2 + a1^2."""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        r = fp_sqrt(a0)
        return (r, 0) if r is not None else (0, fp_sqrt(-a0))
    n = fp_sqrt(a0 * a0 + a1 * a1)
    if n is None:
        return None
    for s in (n, -n % P):
        r = fp_sqrt((a0 + s) * HALF)
        if r:
            cand = (r, a1 * pow(2 * r, -1, P) % P)
            if o.f2_sqr(cand) == (a0, a1):
                return cand
    return None


def y_from_x(x):
    """a y with (x, y) on the curve, from y^2 = (1 + x^2) / (1 - d x^2); None when there is none"""
    x2 = o.f2_sqr(x)
    den = o.f2_sub(o.F2_ONE, o.f2_mul(o.d, x2))
    if den == (0, 0):
        return None
    y = f2_sqrt(o.f2_mul(o.f2_add(o.F2_ONE, x2), o.f2_inv(den)))
    if y is not None:
        assert o.PointOnCurve((x, y))
    return y


# ---- the group law outside the subgroup ---------------------------------------------------------------------------------------
def scalar_mul(k, pt):
    """affine [k]pt by plain double-and-add on the oracle's DBL / ADD (complete formulas: any point of the curve, any k >= 0).
    MUL_windowed reduces its scalar modulo N and MUL_endo assumes the subgroup, so neither can be used for torsion."""
    if k == 0:
        return NEUTRAL
    base = o.R1toR2(o.AffineToR1(*pt))
    acc = o.AffineToR1(*pt)
    for bit in bin(k)[3:]:
        acc = o.DBL(acc)
        if bit == "1":
            acc = o.ADD(acc, base)
    return o.R1toAffine(acc)


def point_add(a, b):
    return o.R1toAffine(o.ADD(o.AffineToR1(*a), o.R1toR2(o.AffineToR1(*b))))


def order_in_392(pt):
    """the order of a point of the 392-torsion"""
    for k in (1, 2, 4, 7, 8, 14, 28, 49, 56, 98, 196, 392):
        if scalar_mul(k, pt) == NEUTRAL:
            return k
    raise AssertionError("not in the 392-torsion")


def y_string(y0, y1, s):
    return y0.to_bytes(16, "little") + (y1 | (s << 127)).to_bytes(16, "little")


def encode(pt):
    return bytes(o.encode(*pt))


def outcome(b):
    """what the oracle's decode does with a string: ("ok", point) or (exception type name, message)"""
    try:
        return "ok", o.decode(b)
    except Exception as exc:
        return type(exc).__name__, str(exc)


def unique(members):
    seen, out = set(), []
    for label, v in members:
        if v not in seen:
            seen.add(v)
            out.append((label, v))
    assert len({label for label, _ in out}) == len(out)
    return out


def _signs(label, x, y, with_y=True):
    out = []
    for sx, xx in (("+x", x), ("-x", o.f2_neg(x))):
        for sy, yy in ((" +y", y), (" -y", o.f2_neg(y))) if with_y else (("", y),):
            out.append(("%s, %s%s" % (label, sx, sy), (xx, yy)))
    return out


# ---- the families -------------------------------------------------------------------------------------------------------------
def imaginary_x():
    """x = (0, x1): decode of the encoding reaches t = 2 (t0 + t3) with t0 != 0 and t3 = p - t0, a zero that is not the integer 0, and
    refuses it as the reference does (AttributeError); encode takes the sign from x1.  x1 and p - x1 both occur, so half the members
    have bit 126 of x1 set.  x1 = +-1, the only edge
    words with a root, give the two points of order 4 (y = 0); the two x1 nearest above 2^126 that have a root bring, with their negatives, the
    sign bit's boundary; the point of order 2 is added."""
    rng = random.Random(9100)
    out, count = [], 0
    while count < 40:
        x1 = rng.randrange(1, P)
        y = y_from_x((0, x1))
        if y is not None:
            out += _signs("seeded imaginary x %d" % count, (0, x1), y)
            count += 1
    for e in E_X:
        y = y_from_x((0, e))
        if y is not None:
            out += _signs("imaginary x1 = %s%s" % (word_name(e), ", order 4" if y == (0, 0) else ""), (0, e), y)
    near = [e for e in range(HALF, HALF + 64) if y_from_x((0, e)) is not None][:2]       # 2^126 itself has no root: the nearest that have
    for e in near:
        out += _signs("imaginary x1 = 2^126%+d" % (e - HALF), (0, e), y_from_x((0, e)))
    out.append(("order 2", ((0, 0), (P - 1, 0))))
    return unique(out)


def real_x():
    """x = (x0, 0): decodes and round-trips; on the way t1 = 0, x.im = 0 and the conjugate candidate equals the first"""
    rng = random.Random(9200)
    out, count = [], 0
    while count < 40:
        x0 = rng.randrange(1, P)
        y = y_from_x((x0, 0))
        if y is not None:
            out += _signs("seeded real x %d" % count, (x0, 0), y, with_y=False)
            count += 1
    for e in E_X:
        y = y_from_x((e, 0))
        if y is not None:
            out += _signs("real x0 = %s" % word_name(e), (e, 0), y, with_y=False)
    return unique(out)


def sign_boundary():
    """one half of x next to 0, to the sign bit or to p, the other seeded: four points for each edge word and half"""
    rng = random.Random(9300)
    out = []
    for half in (0, 1):
        for e in E_X:
            count = 0
            while count < 4:
                r = rng.randrange(1, P)
                x = (e, r) if half == 0 else (r, e)
                y = y_from_x(x)
                if y is not None:
                    out.append(("sign boundary x%d = %s, seeded x%d %d" % (half, word_name(e), 1 - half, count), (x, y)))
                    count += 1
    return unique(out)


def subfield_y():
    """strings with y = (v, 0) and y = (0, v): 150 seeded v and the edge words each, both values of the sign bit; and y in {0, +-1, +-i}"""
    rng = random.Random(9400)
    out = []
    for name, y in (("0", (0, 0)), ("1", (1, 0)), ("-1", (P - 1, 0)), ("i", (0, 1)), ("-i", (0, P - 1))):
        for s in (0, 1):
            out.append(("constant y = %s, sign bit %d" % (name, s), y_string(y[0], y[1], s)))
    for half in (0, 1):
        vs = [("seeded v %d" % k, rng.randrange(P)) for k in range(150)] + [("v = " + word_name(e), e) for e in E_Y]
        for name, v in vs:
            for s in (0, 1):
                out.append(("%s: y = %s, sign bit %d" % (name, "(v, 0)" if half == 0 else "(0, v)", s), y_string(*((v, 0) if half == 0 else (0, v)), s)))
    return unique(out)


def _first_string(rng, want):
    """a seeded string whose outcome is `want` ("ok" or a message)"""
    while True:
        b = y_string(rng.randrange(P), rng.randrange(P), rng.randrange(2))
        kind, what = outcome(b)
        if want in (kind, what):
            return b


def edge_words_y():
    """strings with one half of y on a limb, sign or fold boundary and the other seeded; and the refused class -- y0 = p, y1 = p, bit 127
    of y0 set -- laid over strings that would otherwise be t == 0, off the curve and fine, which are members themselves ("underneath")"""
    rng = random.Random(9500)
    out = []
    for e in E_Y:
        for half in (0, 1):
            for s in (0, 1):
                r = rng.randrange(P)
                out.append(("y%d = %s, seeded y%d, sign bit %d" % (half, word_name(e), 1 - half, s), y_string(*((e, r) if half == 0 else (r, e)), s)))
    under = [("t == 0 (a seeded imaginary x)", encode(imaginary_x()[0][1])), ("off the curve", _first_string(rng, "Point not on curve")),
             ("fine", _first_string(rng, "ok"))]
    for name, b in under:
        out.append(("underneath: " + name, b))
        for s in (0, 1):
            body = bytearray(b)
            body[15] |= 0x80
            body[31] = (body[31] & 0x7F) | (s << 7)
            out.append(("refused: bit 127 of y0 over %s, sign bit %d" % (name, s), bytes(body)))
    # y0 = p and y1 = p: the residue underneath is 0.  (0, 0), (1, 0), (-1, 0) are t == 0; the others by search
    def half_zero(half, want):
        while True:
            v = rng.randrange(P)
            if want in outcome(y_string(*((0, v) if half == 0 else (v, 0)), 0)):
                return v
    for half in (0, 1):
        others = [("t == 0 (y = 0)", 0)]
        if half == 1:
            others += [("t == 0 (y = 1)", 1), ("t == 0 (y = -1)", P - 1)]
        others += [("off the curve", half_zero(half, "Point not on curve")), ("fine", half_zero(half, "ok"))]
        for name, v in others:
            out.append(("underneath: y%d = 0 of %s" % (half, name), y_string(*((0, v) if half == 0 else (v, 0)), 0)))
            for s in (0, 1):
                out.append(("refused: y%d = p over %s, sign bit %d" % (half, name, s), y_string(*((P, v) if half == 0 else (v, P)), s)))
    for s in (0, 1):
        out.append(("refused: y0 = y1 = p, sign bit %d" % s, y_string(P, P, s)))
    return unique(out)


def torsion():
    """T = [N]Q for seeded decodable strings Q until each of the orders 7, 14, 28 and 56 has three members; the points of order 1, 2 and
    4; and points outside the 392-torsion and outside the subgroup, for which DH succeeds: the first three Q, and Q + the point of order 2"""
    rng = random.Random(9600)
    out, seen, full, k = [], {}, [], 0
    while any(seen.get(n, 0) < 3 for n in (7, 14, 28, 56)):
        kind, q = outcome(y_string(rng.randrange(P), rng.randrange(P), rng.randrange(2)))
        if kind != "ok":
            continue
        t = scalar_mul(N, q)
        n = order_in_392(t)
        seen[n] = seen.get(n, 0) + 1
        out.append(("seeded torsion %d: order %d" % (k, n), t))
        if len(full) < 6:
            full.append(("seeded full order %d: Q" % k, q))
            full.append(("seeded full order %d: Q + the point of order 2" % k, point_add(q, ((0, 0), (P - 1, 0)))))
        k += 1
    out += [("order 1", NEUTRAL), ("order 2", ((0, 0), (P - 1, 0))), ("order 4: x = i", ((0, 1), (0, 0))), ("order 4: x = -i", ((0, P - 1), (0, 0)))]
    return unique(out + full)


@functools.lru_cache(maxsize=None)
def _subgroup_search():
    """points OF THE SUBGROUP of order N with x0 = 0 or x1 = 0.  One point in 392 with such an x lies in the subgroup ([N]P is the neutral
    point), so a seeded search finds them: two for each half, and their negatives.  These are the points a pipeline's own output can be."""
    out = []
    for half in (0, 1):
        rng = random.Random(9650 + half)
        count = 0
        while count < 2:
            v = rng.randrange(1, P)
            x = (0, v) if half == 0 else (v, 0)
            y = y_from_x(x)
            if y is not None and scalar_mul(N, (x, y)) == NEUTRAL:
                out += _signs("seeded subgroup point %d with x%d = 0" % (count, half), x, y, with_y=False)
                count += 1
    return tuple(out)


def subgroup_zero_half():
    return list(_subgroup_search())                  # the search costs a second: done once


def subgroup_pipelines():
    """(label, S, m, P, Pdh, k, l, Pdm) for every S above and a seeded odd m, k, l: P = [1/m]S, Pdh = [1/(392 m)]S and Pdm = [1/l](S - [k]G)
    (inverses modulo N), all in the subgroup, so that MUL_*(m, P), DH_*(m, Pdh) and [k]G + [l]Pdm are S: what a ladder, the DH wrapper
    and the double-scalar sum hand to encode with a Z that is not 1"""
    rng = random.Random(9660)
    g = (o.Gx, o.Gy)
    out = []
    for label, s in subgroup_zero_half():
        m, k, l = (rng.getrandbits(256) | 1 for _ in range(3))
        kg = scalar_mul(k % N, g)
        diff = point_add(s, (o.f2_neg(kg[0]), kg[1]))
        out.append((label, s, m, scalar_mul(pow(m, -1, N), s), scalar_mul(pow(392 * m, -1, N), s), k, l, scalar_mul(pow(l, -1, N), diff)))
    return out


PREIMAGE_MS = (3, 5)


def preimages():
    """(label, P, m, S): S from the first three families and P = [1/m mod 392 N]S, so that [m]P = S.  3 and 5 are odd and below N, so
    MUL_windowed multiplies by exactly m and a pipeline emits, from a Z that is not 1, a point with a half of x that is 0"""
    out = []
    for fam in (imaginary_x(), real_x(), sign_boundary()):
        fam = [(label, s) for label, s in fam if "order" not in label]
        picks = fam[:2] + fam[len(fam) // 2:len(fam) // 2 + 2] + fam[-2:]
        for j, (label, s) in enumerate(picks):
            m = PREIMAGE_MS[j % 2]
            out.append(("[1/%d] %s" % (m, label), scalar_mul(pow(m, -1, ORDER), s), m, s))
    return out


POINT_FAMILIES = ("imaginary_x", "real_x", "sign_boundary", "torsion", "subgroup_zero_half")
STRING_FAMILIES = ("subfield_y", "edge_words_y")
_cache = {}


def families():
    """{name: members} for the seven families above and "preimages" (label, P), in a fixed order; built once"""
    if not _cache:
        for name in POINT_FAMILIES + STRING_FAMILIES:
            _cache[name] = globals()[name]()
        _cache["preimages"] = [(label, p) for label, p, _, _ in preimages()]
    return _cache


def all_strings():
    """(family, label, 32 bytes) of every member: the strings as they are, the points through the oracle's encode"""
    out = []
    for name, members in families().items():
        for label, v in members:
            out.append((name, label, v if isinstance(v, bytes) else encode(v)))
    return out


def on_curve_members():
    """(family, label, point) of every member that is a point"""
    return [(name, label, v) for name, members in families().items() for label, v in members if not isinstance(v, bytes)]


DH_SAMPLE = 40


def dh_rows():
    """(family, label, string, seeded scalar): the rows DH_* is recorded for -- every torsion member, subgroup point and preimage and a sample of 40
    strings spread over the other families"""
    rows = all_strings()
    whole = ("torsion", "subgroup_zero_half", "preimages")
    rest = [r for r in rows if r[0] not in whole]
    step = len(rest) // DH_SAMPLE
    picked = [r for r in rows if r[0] in whole] + rest[::step][:DH_SAMPLE]
    rng = random.Random(9700)
    return [(name, label, b, rng.getrandbits(256)) for name, label, b in picked]
