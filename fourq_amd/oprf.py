"""The oblivious PRF on `bytes`, computed on the GPU through the process-wide engine (fourq_oprf_* of include/fourq_amd.h, where the
construction is written out): the client blinds the point its input hashes to, the server multiplies by its key, the client unblinds and
hashes.

    r, blinded = blind(msg, dst)                 client; r is the secret blind (an int), drawn with `secrets` unless given
    evaluated = evaluate(key, blinded)           server; key: an int
    out = finalize(msg, dst, r, evaluated)       client; 64 bytes
    out == evaluate_direct(key, msg, dst)        what the key holder computes on its own

The `_many` forms take lists and make one batched call each.  The suite is this project's own (RFC 9497 registers none for FourQ); `dst`
is the caller's domain separation tag, 1..255 bytes.  A row the library marks (a blind that is 0 mod N, an element that does not decode,
a key that is 0 mod N) raises ValueError.  There is no CPU fallback.
"""
import secrets

import numpy as np

from . import codec
from .constants import N
from .engine import default_engine

# one fixed run of the protocol as the CPU restatement of the construction (tests/oprf_ref.py) gives it: data, for the self-tests
KAT_DST = b"FourQ-OPRF-V01-KAT"
KAT_MSG = b"correct horse battery staple"
KAT_BLIND = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF
KAT_KEY = 0x0123456789ABCDEF0FEDCBA9876543211032547698BADCFEEFCDAB8967452301
KAT_BLINDED = "926025809ccc8f0f878834cf14f93239bb47a3ce46e4502b7582401395191324"
KAT_EVALUATED = "1e869adc8ed18a52d76086c37088f1494e51e3a609395bf84bbb6f0b9297b3b0"
KAT_OUTPUT = ("0b7404b000691cda6f752d302fd757f775c2d10bce22560d13ef14eb21d0b151"
              "bdaa1326735963e8b32d002d0d4ad35890110d6ef7f3bab0cd9e3babbac81f9a")


def _rows32(items):
    rows = [bytes(b) for b in items]
    if any(len(b) != 32 for b in rows):
        raise ValueError("an encoded element is 32 bytes")
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), 32)


def _checked(out, status, what):
    bad = np.flatnonzero(status)
    if len(bad):
        raise ValueError("%s: row %d has status %d (include/fourq_amd.h, \"oblivious PRF\")" % (what, int(bad[0]), int(status[bad[0]])))
    return [r.tobytes() for r in out]


def blind_many(msgs, dst, rs=None):
    """(blinds, 32-byte blinded elements), one per message; `rs`: the blinds to use (ints), fresh ones from `secrets` when None."""
    msgs = [bytes(m) for m in msgs]
    rs = [1 + secrets.randbelow(N - 1) for _ in msgs] if rs is None else [int(r) for r in rs]
    if len(rs) != len(msgs):
        raise ValueError("one blind per message")
    if not msgs:
        return [], []
    matrix, lens = codec.pack_messages(msgs)
    out, status = default_engine().oprf_blind(matrix, codec.pack_scalars(rs), lens, dst=dst)
    return rs, _checked(out, status, "blind")


def blind(msg, dst, r=None):
    rs, out = blind_many([msg], dst, None if r is None else [r])
    return rs[0], out[0]


def evaluate_many(key, blinded):
    """The server's step on a list of 32-byte blinded elements, one key for all."""
    blinded = list(blinded)
    if not blinded:
        return []
    out, status = default_engine().oprf_evaluate(codec.pack_scalars([int(key)])[0], _rows32(blinded))
    return _checked(out, status, "evaluate")


def evaluate(key, blinded32):
    return evaluate_many(key, [blinded32])[0]


def finalize_many(msgs, dst, rs, evaluated):
    """The 64-byte PRF outputs from the messages, their blinds and the server's answers."""
    msgs, rs, evaluated = [bytes(m) for m in msgs], [int(r) for r in rs], list(evaluated)
    if not len(msgs) == len(rs) == len(evaluated):
        raise ValueError("one blind and one evaluated element per message")
    if not msgs:
        return []
    matrix, lens = codec.pack_messages(msgs)
    out, status = default_engine().oprf_finalize(matrix, codec.pack_scalars(rs), _rows32(evaluated), lens, dst=dst)
    return _checked(out, status, "finalize")


def finalize(msg, dst, r, evaluated32):
    return finalize_many([msg], dst, [r], [evaluated32])[0]


def evaluate_direct_many(key, msgs, dst):
    msgs = [bytes(m) for m in msgs]
    if not msgs:
        return []
    matrix, lens = codec.pack_messages(msgs)
    out, status = default_engine().oprf_eval(codec.pack_scalars([int(key)])[0], matrix, lens, dst=dst)
    return _checked(out, status, "evaluate_direct")


def evaluate_direct(key, msg, dst):
    return evaluate_direct_many(key, [msg], dst)[0]
