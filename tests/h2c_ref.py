"""Hash-to-curve as include/fourq_amd.h writes it out ("bytes to a point"), restated over the oracle modules: hashlib for SHA-512, Python
ints modulo p, oracle/curve4q_oracle.py for GF(p^2) and the points.  A helper for the hash-to-curve tests, not the code under test.

RFC 9380's construction for FourQ -- expand_message_xmd with SHA-512 (section 5.3.1), hash_to_field with m = 2, L = 32 (5.2), the
Montgomery-form Elligator 2 (6.7.1) on K t^2 = s^3 + J s^2 + s, the rational map of appendix D.1 and the reference's x392 chain.  The
constants J, K are DERIVED here from d (nothing is copied from fourq_amd/constants.py, which tests/test_h2c_oracle.py pins against this
file); Z = 2 + i.  The square root is written differently from the device's (exponent (p^2 + 7) / 16-free: a norm and two GF(p) roots, each
CHECKED by squaring), and sgn0 makes the result independent of the route.

REACHED counts how often the exceptional rules fired since import: "inv0" (1 + Z u^2 == 0) and "neutral" (t (s + 1) == 0 in the rational map).
"""
import hashlib

import curve4q_oracle as o

P = o.P127
ONE, ZERO = (1, 0), (0, 0)
Z = (2, 1)
RO, NU = 0, 1
MAX_DST = 255
# K t^2 = s^3 + J s^2 + s  <->  a x^2 + y^2 = 1 + d x^2 y^2 with a = -1:  J = 2 (a + d) / (a - d), K = 4 / (a - d)   (RFC 9380 appendix D.1)
_A = o.f2_neg(ONE)
_AMD_INV = o.f2_inv(o.f2_sub(_A, o.d))
J = o.f2_mul(o.f2_mul((2, 0), o.f2_add(_A, o.d)), _AMD_INV)
K = o.f2_mul((4, 0), _AMD_INV)
K_INV = o.f2_inv(K)
JK = o.f2_mul(J, K_INV)                    # J / K
IK2 = o.f2_sqr(K_INV)                      # 1 / K^2
REACHED = {"inv0": 0, "neutral": 0}


# ---- RFC 9380 section 5: bytes -> field elements ----------------------------------------------------------------------------------
def expand_message_xmd(msg, dst, len_in_bytes):
    msg, dst = bytes(msg), bytes(dst)
    if not 1 <= len(dst) <= MAX_DST:
        raise ValueError("DST must be 1..255 bytes")
    ell = (len_in_bytes + 63) // 64
    assert 1 <= ell <= 255 and len_in_bytes <= 65535
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha512(bytes(128) + msg + len_in_bytes.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    b = [hashlib.sha512(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha512(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:len_in_bytes]


def hash_to_field(msg, dst, mode):
    """[u_0, u_1] (RO) or [u_0] (NU); u_i = (e_i0, e_i1) canonical."""
    count = 2 if mode == RO else 1
    uniform = expand_message_xmd(msg, dst, count * 64)
    e = [int.from_bytes(uniform[32 * k:32 * k + 32], "big") % P for k in range(2 * count)]
    return [(e[2 * i], e[2 * i + 1]) for i in range(count)]


# ---- GF(p^2) helpers the oracle does not have --------------------------------------------------------------------------------------
def fp_is_square(x):
    return x % P == 0 or pow(x, (P - 1) // 2, P) == 1


def fp_sqrt(x):
    r = pow(x, (P + 1) // 4, P)
    assert r * r % P == x % P, "not a square of GF(p)"
    return r


def norm(a):
    return (a[0] * a[0] + a[1] * a[1]) % P


def is_square(a):
    """a is a square of GF(p^2) iff its norm is a square of GF(p) (zero included)."""
    return fp_is_square(norm(a))


def sqrt(a):
    """some square root of a square a = (a0, a1): x0^2 = (a0 +- |a|) / 2, x1 = a1 / (2 x0); checked."""
    a = (a[0] % P, a[1] % P)
    half = (P + 1) // 2
    if a[1] == 0:
        r = (fp_sqrt(a[0]), 0) if fp_is_square(a[0]) else (0, fp_sqrt(P - a[0]))
    else:
        s = fp_sqrt(norm(a))
        t = (a[0] + s) * half % P
        if not fp_is_square(t):
            t = (a[0] - s) * half % P
        x0 = fp_sqrt(t)                                     # t != 0 because a1 != 0
        r = (x0, a[1] * pow(2 * x0, P - 2, P) % P)
    assert o.f2_sqr(r) == a
    return r


def sgn0(a):
    """RFC 9380 section 4.1 for m = 2, on canonical residues."""
    re, im = a[0] % P, a[1] % P
    return (re & 1) | ((1 if re == 0 else 0) & (im & 1))


def inv0(a):
    return ZERO if (a[0] % P, a[1] % P) == ZERO else o.f2_inv(a)


def canon(a):
    return (a[0] % P, a[1] % P)


# ---- RFC 9380 section 6.7.1 and appendix D.1 -------------------------------------------------------------------------------------------
def g_of(x):
    """x^3 + (J/K) x^2 + x / K^2"""
    x2 = o.f2_sqr(x)
    return o.f2_add(o.f2_add(o.f2_mul(x2, x), o.f2_mul(JK, x2)), o.f2_mul(x, IK2))


def elligator2_candidates(u):
    t = inv0(o.f2_add(ONE, o.f2_mul(Z, o.f2_sqr(u))))
    x1 = o.f2_neg(o.f2_mul(JK, t))
    if canon(t) == ZERO:
        REACHED["inv0"] += 1
        x1 = o.f2_neg(JK)
    x2 = o.f2_sub(o.f2_neg(x1), JK)
    return canon(x1), canon(x2)


def map_to_montgomery(u):
    """(s, t, branch) on K t^2 = s^3 + J s^2 + s; branch 1: x1 was taken, 2: x2."""
    x1, x2 = elligator2_candidates(u)
    gx1 = g_of(x1)
    if is_square(gx1):
        x, y, branch = x1, sqrt(gx1), 1
        if sgn0(y) != 1:
            y = o.f2_neg(y)
    else:
        gx2 = g_of(x2)
        x, y, branch = x2, sqrt(gx2), 2
        if sgn0(y) != 0:
            y = o.f2_neg(y)
    return canon(o.f2_mul(x, K)), canon(o.f2_mul(y, K)), branch


def montgomery_to_edwards(s, t):
    den = o.f2_mul(t, o.f2_add(s, ONE))
    if canon(den) == ZERO:
        REACHED["neutral"] += 1
        return ZERO, ONE
    return canon(o.f2_mul(s, o.f2_inv(t))), canon(o.f2_mul(o.f2_sub(s, ONE), o.f2_inv(o.f2_add(s, ONE))))


def map_to_curve(u):
    """Elligator 2 + the rational map: an affine point of E, NO cofactor clearing.  u: any pair of integers."""
    s, t, _ = map_to_montgomery((u[0] % P, u[1] % P))
    return montgomery_to_edwards(s, t)


# ---- points: the oracle's own DBL / ADD ------------------------------------------------------------------------------------------------
def clear_cofactor(A):
    return o.R1toAffine(o.clear_cofactor(o.AffineToR1(*A)))


def add_affine(A, B):
    return o.R1toAffine(o.ADD(o.AffineToR1(*A), o.R1toR2(o.AffineToR1(*B))))


def hash_to_curve_affine(msg, dst, mode=RO):
    u = hash_to_field(msg, dst, mode)
    Q = map_to_curve(u[0])
    if mode == RO:
        Q = add_affine(Q, map_to_curve(u[1]))
    x, y = clear_cofactor(Q)
    return canon(x), canon(y)


def hash_to_curve(msg, dst, mode=RO):
    """32 bytes: encode([392](map(u_0) [+ map(u_1)]))."""
    return bytes(o.encode(*hash_to_curve_affine(msg, dst, mode)))


def u_words(u):
    """4 x u64 little-endian words of u = (re, im)."""
    m = (1 << 64) - 1
    return [u[0] & m, u[0] >> 64, u[1] & m, u[1] >> 64]


def affine_words(A):
    return u_words(A[0]) + u_words(A[1])


# ---- the two inputs where a candidate abscissa is -1/K (s = -1: the rational map's y has no denominator) ---------------------------
def special_inputs():
    """[(u, which)]: u with x1 == -1/K and u with x2 == -1/K.  x1 = -(J/K) / (1 + Z u^2) = -1/K  <=>  Z u^2 = J - 1;
    x2 = Z u^2 x1 = -1/K  <=>  Z u^2 (J - 1) = 1.  Both right-hand sides divided by Z must be squares for u to exist."""
    out = []
    zi = o.f2_inv(Z)
    jm1 = o.f2_sub(J, ONE)
    for which, w in ((1, o.f2_mul(jm1, zi)), (2, o.f2_mul(o.f2_inv(jm1), zi))):
        if is_square(w):
            out.append((sqrt(w), which))
    return out
