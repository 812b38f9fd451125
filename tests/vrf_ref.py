"""The verifiable random function as include/fourq_amd.h writes it out ("verifiable random function"), restated over the oracle modules:
hashlib for SHA-512, tests/h2c_ref.py for hash to curve and the x392 chain, tests/sig_ref.py for the keys and decode's statuses,
tests/keyset_ref.py for the key set, oracle/curve4q_oracle.py for MUL_endo, ADD, encode and decode.  A helper for the VRF tests, not the code
under test.

One row per (key, alpha).  Every function that stands for a library call returns, per row, what the library reports: verify gives
(ok, status, beta64) with beta64 all zero unless ok, proof_to_hash gives (beta64, status) with beta64 all zero unless the status is 0.
"""
import hashlib

import curve4q_oracle as o
import h2c_ref
import keyset_ref
import sig_ref

N = o.N
INV392 = pow(392, -1, N)
DECODE_BASE, SIG_S_RANGE, GAMMA_NEUTRAL = 16, 32, 128
KEYSET_NOT_ORDER_N, KEYSET_ID_RANGE = keyset_ref.KEYSET_NOT_ORDER_N, keyset_ref.KEYSET_ID_RANGE
GEN = (o.Gx, o.Gy)
NEUTRAL32 = bytes([1] + [0] * 31)
ZERO_BETA = bytes(64)
REFUSED_NEUTRAL = DECODE_BASE + sig_ref.DECODE_REF_ATTRIBUTE_ERROR        # what the sum of two says of an Hpt that is the neutral point

H, LE = sig_ref.H, sig_ref.LE


def enc(P):
    return bytes(o.encode(P[0], P[1]))


def tail(label, dst):
    assert 1 <= len(dst) <= 255 and len(label) == 9
    return label + bytes(dst) + bytes([len(dst)])


def mul(m, A):
    """R1toAffine(MUL_endo(m, AffineToR1(A)))"""
    return o.R1toAffine(o.MUL_endo(m, o.AffineToR1(A[0], A[1])))


def point_sum(scalars, points):
    """R1toAffine(sum of MUL_endo(k, AffineToR1(P))) by the complete addition, as fourq_msm_* and fourq_double_mul_* define it"""
    acc = None
    for k, P in zip(scalars, points):
        T = o.MUL_endo(k, o.AffineToR1(P[0], P[1]))
        acc = T if acc is None else o.ADD(acc, o.R1toR2(T))
    return o.R1toAffine(acc)


def hash_point(pk32, alpha, dst):
    """Hpt: hash to curve, RO mode, under dst, of the string pk32 || alpha"""
    return h2c_ref.hash_to_curve_affine(bytes(pk32) + bytes(alpha), dst, h2c_ref.RO)


def challenge(pk32, h32, gamma32, u32, v32, dst):
    return LE(H(bytes(pk32) + h32 + bytes(gamma32) + u32 + v32 + tail(b"VrfVerify", dst))) % N


def output(w32, dst):
    return H(w32 + tail(b"VrfOutput", dst))


def secret_scalars(sk32, h32):
    """(x, r): x = LE(k[0:32]) unreduced, r = LE(H(k[32:64] || h32)) mod N"""
    k = H(sk32)
    return LE(k[:32]), LE(H(k[32:] + h32)) % N


def prove(sk32, pk32, alpha, dst, shift=None):
    """proof96.  shift: a point T the dishonest prover adds to Gamma before hashing the challenge (T of the 392-torsion is accepted)"""
    Hpt = hash_point(pk32, alpha, dst)
    h32 = enc(Hpt)
    x, r = secret_scalars(sk32, h32)
    Gamma = mul(x, Hpt)
    if shift is not None:
        Gamma = o.R1toAffine(o.ADD(o.AffineToR1(*Gamma), o.R1toR2(o.AffineToR1(*shift))))
    gamma32 = enc(Gamma)
    u32, v32 = enc(mul(r, GEN)), enc(mul(r, Hpt))
    c = challenge(pk32, h32, gamma32, u32, v32, dst)
    s = (r - c * x) % N
    return gamma32 + c.to_bytes(32, "little") + s.to_bytes(32, "little")


def cleared(gamma32):
    """(W, w32, status): W = [392]decode(gamma32) by the x392 chain; status: the decode code of gamma32, else GAMMA_NEUTRAL for a neutral W"""
    st, Gamma = sig_ref.decode_status(bytes(gamma32))
    if st:
        return None, bytes(32), st
    W = h2c_ref.clear_cofactor(Gamma)
    w32 = enc(W)
    return W, w32, (GAMMA_NEUTRAL if w32 == NEUTRAL32 else 0)


def verify(pk32, alpha, proof96, dst):
    """(ok, status, beta64) of one row of fourq_vrf_verify (the clamped message of the _dev call has no counterpart here)"""
    pk32, proof96 = bytes(pk32), bytes(proof96)
    st, Y = sig_ref.decode_status(pk32)
    if st:
        return 0, st, ZERO_BETA
    W, w32, wst = cleared(proof96[:32])
    if wst and wst != GAMMA_NEUTRAL:
        return 0, wst, ZERO_BETA
    c, s = LE(proof96[32:64]), LE(proof96[64:])
    if c >= N or s >= N:
        return 0, SIG_S_RANGE, ZERO_BETA
    if wst:
        return 0, GAMMA_NEUTRAL, ZERO_BETA
    Hpt = hash_point(pk32, alpha, dst)
    h32 = enc(Hpt)
    if h32 == NEUTRAL32:
        return 0, REFUSED_NEUTRAL, ZERO_BETA
    u32 = enc(point_sum([s, c], [GEN, Y]))
    v32 = enc(point_sum([s, c * INV392 % N], [Hpt, W]))
    if challenge(pk32, h32, proof96[:32], u32, v32, dst) != c:
        return 0, 0, ZERO_BETA
    return 1, 0, output(w32, dst)


def verify_keyed(keys, key_id, alpha, proof96, dst):
    """(ok, status, beta64) of one row of fourq_keyset_vrf_verify: an index outside the set, then the key's own status, then verify"""
    st = keyset_ref.row_status(keys, key_id)
    if st:
        return 0, st, ZERO_BETA
    return verify(keys[key_id], alpha, proof96, dst)


def proof_to_hash(proof96, dst):
    """(beta64, status): c and s are not looked at"""
    _, w32, st = cleared(bytes(proof96)[:32])
    return (ZERO_BETA, st) if st else (output(w32, dst), 0)


def flipped(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def soundness_cases(pks, alphas, proofs, dst):
    """An honest batch of at least four rows with distinct keys, tampered with in every way the issue lists.  Yields
    (label, pks, alphas, proofs, dst, rows that must now fail); every other row must still be accepted, with its beta."""
    pks, alphas, proofs = [bytes(p) for p in pks], [bytes(a) for a in alphas], [bytes(p) for p in proofs]
    n = len(proofs)
    assert n >= 4 and len(set(pks)) == n
    last = n - 1

    def with_row(rows, i, value):
        rows = rows[:]
        rows[i] = value
        return rows

    bit = next(k for k in range(256) if sig_ref.decode_status(flipped(proofs[last][:32], k))[0] == 0)        # a Gamma that still decodes
    yield "one flipped bit in gamma", pks, alphas, with_row(proofs, last, flipped(proofs[last], bit)), dst, [last]
    for label, at in (("c", 256), ("s", 512)):
        p = flipped(proofs[last], at)
        assert LE(p[32:64]) < N and LE(p[64:]) < N
        yield "one flipped bit in " + label, pks, alphas, with_row(proofs, last, p), dst, [last]
    moved = with_row(with_row(proofs, 0, proofs[1]), 1, proofs[0])
    yield "a proof moved to another row", pks, alphas, moved, dst, [0, 1]
    i = next(k for k in range(n) if len(alphas[k]) >= 2)
    yield "one changed byte of alpha", pks, with_row(alphas, i, flipped(alphas[i], 8 * (len(alphas[i]) - 1))), proofs, dst, [i]
    yield "alpha one byte shorter", pks, with_row(alphas, i, alphas[i][:-1]), proofs, dst, [i]
    yield "a pk32 that decodes but is another key", with_row(pks, 2, pks[3]), alphas, proofs, dst, [2]
    yield "one flipped bit in dst", pks, alphas, proofs, flipped(dst, 0), list(range(n))
