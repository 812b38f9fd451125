"""The oblivious PRF as include/fourq_amd.h writes it out ("oblivious PRF"), restated over the oracle modules: hashlib for SHA-512,
tests/h2c_ref.py for G(msg), oracle/curve4q_oracle.py for MUL_endo, DH_endo, encode and decode, and Python's pow for 1 / r mod N.
A helper for the OPRF tests, not the code under test.

Every function returns (bytes, status) as the library reports a row: the output row is all zero unless status is 0.
"""
import hashlib

import curve4q_oracle as o
import h2c_ref

N = o.N
BLIND_ZERO, DH_NEUTRAL, DECODE_BASE = 48, 2, 16
DECODE_RESERVED_BIT, DECODE_NOT_ON_CURVE, DECODE_REF_ATTRIBUTE_ERROR = 1, 2, 3


def G(msg, dst):
    return h2c_ref.hash_to_curve_affine(msg, dst, h2c_ref.RO)


def mul_affine(m, A):
    return o.R1toAffine(o.MUL_endo(m, o.AffineToR1(A[0], A[1])))


def decode_status(b32):
    """(point or None, FOURQ_DECODE_*) as fourq_decode_batch reports the reference's exceptions"""
    try:
        return o.decode(b32), 0
    except AttributeError:
        return None, DECODE_REF_ATTRIBUTE_ERROR
    except Exception as exc:
        return None, DECODE_NOT_ON_CURVE if "not on curve" in str(exc) else DECODE_RESERVED_BIT


def final_hash(e32, msg, dst):
    """F(E, msg) = SHA-512(E || msg || "Finalize" || dst || I2OSP(len(dst), 1))"""
    assert len(e32) == 32 and 1 <= len(dst) <= 255
    return hashlib.sha512(bytes(e32) + bytes(msg) + b"Finalize" + bytes(dst) + bytes([len(dst)])).digest()


def blind(msg, dst, r):
    if r % N == 0:
        return bytes(32), BLIND_ZERO
    return bytes(o.encode(*mul_affine(r, G(msg, dst)))), 0


def evaluate(key, blinded32):
    P, st = decode_status(blinded32)
    if st:
        return bytes(32), DECODE_BASE + st
    try:
        return bytes(o.encode(*o.DH_endo(key, P))), 0
    except Exception as exc:
        return bytes(32), DH_NEUTRAL if "neutral" in str(exc) else 1


def finalize(msg, dst, r, evaluated32):
    Z, st = decode_status(evaluated32)
    if st:
        return bytes(64), DECODE_BASE + st
    if r % N == 0:
        return bytes(64), BLIND_ZERO
    E = bytes(o.encode(*mul_affine(pow(r % N, -1, N), Z)))
    return final_hash(E, msg, dst), 0


def evaluate_direct(key, msg, dst):
    try:
        E = bytes(o.encode(*o.DH_endo(key, G(msg, dst))))
    except Exception:
        return bytes(64), DH_NEUTRAL
    return final_hash(E, msg, dst), 0
