"""The signature scheme of include/fourq_amd.h ("signatures from bytes") restated over the oracle modules: hashlib for SHA-512, Python
ints modulo N, oracle/curve4q_oracle.py for the points.  A helper for the signature tests, not the code under test.

`batch_*` are the same functions with the point work done by the C oracle (oracle/oracle_c.py), so that GPU tests can afford 2^16 rows;
tests/test_sig_oracle.py pins them against the restatement.
"""
import hashlib

import numpy as np

import curve4q_oracle as o

N = o.N
G1 = o.AffineToR1(o.Gx, o.Gy)
SIG_S_RANGE, BYTES_DECODE_BASE = 32, 16
DECODE_RESERVED_BIT, DECODE_NOT_ON_CURVE, DECODE_REF_ATTRIBUTE_ERROR = 1, 2, 3


def H(b):
    return hashlib.sha512(bytes(b)).digest()


def LE(b):
    return int.from_bytes(bytes(b), "little")


def mul_g_encoded(m):
    return bytes(o.encode(*o.R1toAffine(o.MUL_endo(m, G1))))


def keygen(sk):
    return mul_g_encoded(LE(H(sk)[:32]))


def nonce(sk, msg):
    return LE(H(H(sk)[32:] + bytes(msg))) % N


def challenge(R, pk, msg):
    return LE(H(bytes(R) + bytes(pk) + bytes(msg))) % N


def sign(sk, pk, msg):
    k = H(sk)
    r = nonce(sk, msg)
    R = mul_g_encoded(r)
    s = (r - LE(k[:32]) * challenge(R, pk, msg)) % N
    return R + s.to_bytes(32, "little")


def decode_status(pk):
    """0, or BYTES_DECODE_BASE + FOURQ_DECODE_* for the exception the oracle's decode raises; and the point."""
    try:
        return 0, o.decode(pk)
    except AttributeError:
        return BYTES_DECODE_BASE + DECODE_REF_ATTRIBUTE_ERROR, None
    except Exception as exc:
        return BYTES_DECODE_BASE + (DECODE_NOT_ON_CURVE if "not on curve" in str(exc) else DECODE_RESERVED_BIT), None


def verify(pk, msg, sig):
    """(ok, status) as fourq_sig_verify_batch defines them."""
    st, A = decode_status(pk)
    if st:
        return 0, st                                   # a key that does not decode takes precedence
    s = LE(sig[32:])
    if s >= N:
        return 0, SIG_S_RANGE
    h = challenge(sig[:32], pk, msg)
    P = o.ADD(o.MUL_endo(s, G1), o.R1toR2(o.MUL_endo(h, o.AffineToR1(*A))))
    return (1 if bytes(o.encode(*o.R1toAffine(P))) == bytes(sig[:32]) else 0), 0


# ---- the same with the point work in the C oracle -------------------------------------------------------------------------------
def _mul_g_encoded_batch(ints):
    import oracle_c as oc
    from fourq_amd import codec
    table = oc.table(oc.ENDO, codec.pack_point(G1))
    return oc.encode(oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(ints), None, table)))


def batch_keygen(sks):
    """(n, 32) uint8 public keys of a list of 32-byte secret keys."""
    return _mul_g_encoded_batch([LE(H(sk)[:32]) for sk in sks])


def batch_sign(sks, pks, msgs):
    """(n, 64) uint8 signatures; pks: (n, 32) uint8 or a list of bytes."""
    rs = [nonce(sk, m) for sk, m in zip(sks, msgs)]
    R = _mul_g_encoded_batch(rs)
    out = np.empty((len(sks), 64), dtype=np.uint8)
    out[:, :32] = R
    for i, (sk, m) in enumerate(zip(sks, msgs)):
        s = (rs[i] - LE(H(sk)[:32]) * challenge(R[i].tobytes(), bytes(pks[i]), m)) % N
        out[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8)
    return out
