"""Signatures of registered keys (include/fourq_amd.h, "signatures of registered keys") restated over tests/sig_ref.py and the Python
oracle: the key set's statuses, the order check by plain double-and-add, and the two calls with their precedence of statuses.  A helper
for the key-set tests, nothing from the library under test."""
import curve4q_oracle as o
import sig_ref

N = o.N
KEYSET_NOT_ORDER_N, KEYSET_ID_RANGE = 96, 112
SIG_S_RANGE = sig_ref.SIG_S_RANGE
NEUTRAL_AFFINE = ((0, 0), (1, 0))
NEUTRAL_BYTES = bytes([1] + [0] * 31)
ZERO_ROW = bytes(32)


def plain_mul(k, P):
    """[k]P, canonical affine, for ANY point of the curve and k >= 1: double-and-add with the oracle's DBL and its complete ADD.
    Neither MUL_endo nor MUL_windowed is [k]P outside the subgroup of order N."""
    assert k >= 1
    P1 = o.AffineToR1(*P)
    P2 = o.R1toR2(P1)
    Q = P1
    for bit in bin(k)[3:]:
        Q = o.DBL(Q)
        if bit == "1":
            Q = o.ADD(Q, P2)
    return tuple(tuple(int(c) for c in coord) for coord in o.R1toAffine(Q))


def has_order_n(P):
    return plain_mul(N, P) == NEUTRAL_AFFINE


def key_status(pk):
    """the status byte fourq_keyset_set gives the slot of `pk`"""
    st, A = sig_ref.decode_status(pk)
    if st:
        return st
    return 0 if has_order_n(A) else KEYSET_NOT_ORDER_N


def row_status(keys, key_id):
    return KEYSET_ID_RANGE if key_id >= len(keys) else key_status(keys[key_id])


def verify_keyed(keys, key_id, msg, sig):
    """(ok, status) of fourq_keyset_sig_verify for one row: an index outside the set, then the key's own status, then s >= N (the
    clamped message of the _dev call has no counterpart here: the restatement takes whole messages)"""
    st = row_status(keys, key_id)
    if st:
        return 0, st
    return sig_ref.verify(keys[key_id], msg, sig)


def double_mul_keyed(keys, key_id, k, l):
    """(out32, status) of fourq_keyset_double_mul_bytes for one row"""
    st = row_status(keys, key_id)
    if st:
        return ZERO_ROW, st
    A = o.decode(keys[key_id])
    P = o.ADD(o.MUL_endo(k, sig_ref.G1), o.R1toR2(o.MUL_endo(l, o.AffineToR1(*A))))
    return bytes(bytearray(o.encode(*o.R1toAffine(P)))), 0
