"""The batched DLEQ proofs as include/fourq_amd.h writes them out ("oblivious PRF: proofs"), restated over the oracle modules: hashlib for
SHA-512, tests/oprf_ref.py for decode's statuses and the server's evaluation, oracle/curve4q_oracle.py for MUL_endo, DH_endo, ADD, encode
and decode.  A helper for the DLEQ tests, not the code under test.

A batch is groups x group_size rows laid out group after group; every function that stands for a library call returns, per group, what
the library reports: the output row (all zero unless the status is 0) and the status.
"""
import hashlib

import curve4q_oracle as o
import oprf_ref

N = o.N
DH_NEUTRAL, DECODE_BASE, SIG_S_RANGE, NONCE_ZERO = 2, 16, 32, 80
DECODE_REF_ATTRIBUTE_ERROR = 3
GEN = (o.Gx, o.Gy)
NEUTRAL32 = bytes([1] + [0] * 31)
REFUSED_NEUTRAL = DECODE_BASE + DECODE_REF_ATTRIBUTE_ERROR       # what the next stage's decode says of a composite that is the neutral point


def enc(P):
    return bytes(o.encode(P[0], P[1]))


def tail(label, dst):
    assert 1 <= len(dst) <= 255
    return label + bytes(dst) + bytes([len(dst)])


def le_mod_n(digest):
    return int.from_bytes(digest, "little") % N


def public_key(key):
    """(pk32, status): encode(DH_endo(key, Gen)), the server's evaluation of the generator's encoding"""
    return oprf_ref.evaluate(key, enc(GEN))


def composite_scalar(pk32, c32, d32, j, dst):
    return le_mod_n(hashlib.sha512(bytes(pk32) + bytes(c32) + bytes(d32) + j.to_bytes(4, "big") + tail(b"Composite", dst)).digest())


def challenge(pk32, m32, z32, t2, t3, dst):
    return le_mod_n(hashlib.sha512(bytes(pk32) + m32 + z32 + t2 + t3 + tail(b"Challenge", dst)).digest())


def point_sum(scalars, points):
    """R1toAffine(sum of MUL_endo(k, AffineToR1(P))) by the complete addition, as fourq_msm_* defines it"""
    acc = None
    for k, P in zip(scalars, points):
        T = o.MUL_endo(k, o.AffineToR1(P[0], P[1]))
        acc = T if acc is None else o.ADD(acc, o.R1toR2(T))
    return o.R1toAffine(acc)


def decoded(rows):
    """(points, the largest FOURQ_DECODE_* among the rows)"""
    pairs = [oprf_ref.decode_status(bytes(r)) for r in rows]
    return [p for p, _ in pairs], max(st for _, st in pairs)


def scalars_of(pk32, cs, ds, dst):
    return [composite_scalar(pk32, c, d, j, dst) for j, (c, d) in enumerate(zip(cs, ds))]


def composites_group(pk32, cs, ds, dst):
    """(M32, Z32, status) of one group as fourq_dleq_composites reports it: the verifier's composites"""
    cpts, cst = decoded(cs)
    dpts, dst_code = decoded(ds)
    if max(cst, dst_code):
        return bytes(32), bytes(32), DECODE_BASE + max(cst, dst_code)
    d = scalars_of(pk32, cs, ds, dst)
    return enc(point_sum(d, cpts)), enc(point_sum(d, dpts)), 0


def prove_group(key, cs, ds, nonce, dst, parts=False):
    """(proof64, status) of one group; with `parts` also {"d", "M32", "Z32"} (None where the group is refused)"""
    def refused(st):
        return (bytes(64), st, None) if parts else (bytes(64), st)
    pk32, _ = public_key(key)                        # all zero when key = 0 mod N: the group is refused below, whatever was hashed
    cpts, cst = decoded(cs)
    if cst:
        return refused(DECODE_BASE + cst)
    if key % N == 0:
        return refused(DH_NEUTRAL)
    d = scalars_of(pk32, cs, ds, dst)
    M = point_sum(d, cpts)
    m32 = enc(M)
    if m32 == NEUTRAL32:
        return refused(REFUSED_NEUTRAL)
    try:
        Z = o.DH_endo(key, M)
    except Exception:
        return refused(DH_NEUTRAL)
    r = nonce % N
    if r == 0:
        return refused(NONCE_ZERO)
    z32 = enc(Z)
    t2 = enc(o.R1toAffine(o.MUL_endo(r, o.AffineToR1(*GEN))))
    t3 = enc(o.R1toAffine(o.MUL_endo(r, o.AffineToR1(M[0], M[1]))))
    c = challenge(pk32, m32, z32, t2, t3, dst)
    s = (r - c * (392 * key % N)) % N
    proof = c.to_bytes(32, "little") + s.to_bytes(32, "little")
    return (proof, 0, {"d": d, "M32": m32, "Z32": z32}) if parts else (proof, 0)


def verify_group(pk32, cs, ds, proof64, dst):
    """(ok, status) of one group"""
    cpts, cst = decoded(cs)
    dpts, dst_code = decoded(ds)
    pk, pkst = oprf_ref.decode_status(bytes(pk32))
    if max(cst, dst_code, pkst):
        return 0, DECODE_BASE + max(cst, dst_code, pkst)
    c, s = int.from_bytes(proof64[:32], "little"), int.from_bytes(proof64[32:], "little")
    if c >= N or s >= N:
        return 0, SIG_S_RANGE
    d = scalars_of(pk32, cs, ds, dst)
    M, Z = point_sum(d, cpts), point_sum(d, dpts)
    m32, z32 = enc(M), enc(Z)
    if NEUTRAL32 in (m32, z32):
        return 0, REFUSED_NEUTRAL
    t2 = enc(point_sum([s, c], [GEN, pk]))
    t3 = enc(point_sum([s, c], [M, Z]))
    return int(challenge(pk32, m32, z32, t2, t3, dst) == c), 0


def soundness_cases(key, pk32, blinded, evaluated, proofs, dst, group_size):
    """An honest batch of at least two groups of at least two rows, tampered with in every way the issue lists.  Yields
    (label, pk32, blinded, evaluated, proofs, dst, groups that must now fail); every other group must still be accepted."""
    blinded, evaluated, proofs = [bytes(b) for b in blinded], [bytes(b) for b in evaluated], [bytes(p) for p in proofs]
    groups = len(proofs)
    assert groups >= 2 and group_size >= 2 and len(blinded) == groups * group_size
    everyone = list(range(groups))

    def flipped(b, bit):
        b = bytearray(b)
        b[bit // 8] ^= 1 << (bit % 8)
        return bytes(b)

    other = evaluated[:]
    other[group_size + 1] = oprf_ref.evaluate((key + 1) % N or 2, blinded[group_size + 1])[0]
    yield "one evaluated row made with another key", pk32, blinded, other, proofs, dst, [1]
    b, e = blinded[:], evaluated[:]
    b[0], b[1], e[0], e[1] = b[1], b[0], e[1], e[0]
    yield "two rows of a group swapped", pk32, b, e, proofs, dst, [0]
    moved = proofs[:]
    moved[0], moved[1] = proofs[1], proofs[0]
    yield "a proof moved to another group", pk32, blinded, evaluated, moved, dst, [0, 1]
    g = groups - 1
    for label, bit in (("c", 0), ("s", 256)):
        p = proofs[:]
        p[g] = flipped(p[g], bit)
        assert int.from_bytes(p[g][:32], "little") < N and int.from_bytes(p[g][32:], "little") < N
        yield "one flipped bit in " + label, pk32, blinded, evaluated, p, dst, [g]
    bit = next(k for k in range(256) if oprf_ref.decode_status(flipped(pk32, k))[1] == 0)        # another key that still decodes
    yield "one flipped bit in pk", flipped(pk32, bit), blinded, evaluated, proofs, dst, everyone
    yield "one flipped bit in dst", pk32, blinded, evaluated, proofs, flipped(dst, 0), everyone


def groups_of(rows, group_size):
    rows = [bytes(r) for r in rows]
    assert group_size > 0 and len(rows) % group_size == 0
    return [rows[i:i + group_size] for i in range(0, len(rows), group_size)]


def composites(pk32, blinded, evaluated, dst, group_size):
    return [composites_group(pk32, cs, ds, dst) for cs, ds in zip(groups_of(blinded, group_size), groups_of(evaluated, group_size))]


def prove(key, blinded, evaluated, nonces, dst, group_size):
    return [prove_group(key, cs, ds, r, dst) for cs, ds, r in zip(groups_of(blinded, group_size), groups_of(evaluated, group_size), nonces)]


def verify(pk32, blinded, evaluated, proofs, dst, group_size):
    return [verify_group(pk32, cs, ds, bytes(p), dst) for cs, ds, p in zip(groups_of(blinded, group_size), groups_of(evaluated, group_size), proofs)]
