"""The oblivious PRF on `bytes`, computed on the GPU through the process-wide engine (fourq_oprf_* of include/fourq_amd.h, where the
construction is written out): the client blinds the point its input hashes to, the server multiplies by its key, the client unblinds and
hashes.

    r, blinded = blind(msg, dst)                 client; r is the secret blind (an int), drawn with `secrets` unless given
    evaluated = evaluate(key, blinded)           server; key: an int
    out = finalize(msg, dst, r, evaluated)       client; 64 bytes
    out == evaluate_direct(key, msg, dst)        what the key holder computes on its own

and, for a server that must show which key it used (fourq_dleq_*, "oblivious PRF: proofs"):

    pk = public_key(key)                                   server, once; published
    proofs = prove(key, blinded, evaluated, dst)           server; one 64-byte proof per group of `group_size` elements
    verify(pk, blinded, evaluated, proofs, dst)            client; one bool per group

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
# ... and the server's proof for that one row as a group of its own (tests/dleq_ref.py); the nonce is used mod N
KAT_PK = "80a21fdd53c30b7d8face9a3ac84ed71398da1370742e725da954747c17d2ef3"
KAT_NONCE = 0x0FEDCBA98765432100112233445566778899AABBCCDDEEFF0123456789ABCDEF
KAT_PROOF = ("018e836db111f52caf1e16d2ca46f93c00b320220bf99705b77486e6236f2600"
             "cf3f328665e4a248fe6bb4726ddb0f582995d183965e674fc8cadb661a7d0e00")


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


def public_key(key):
    """The 32 bytes a server publishes for `key`: its evaluation of the generator's encoding."""
    return default_engine().dleq_public_key(codec.pack_scalars([int(key)])[0]).tobytes()


def _engine_with_comb():
    """the default engine and the comb of the generator, built once per engine: the signature module's"""
    from .schnorrq import _engine
    return _engine()


def _groups(blinded, evaluated, group_size):
    blinded, evaluated = list(blinded), list(evaluated)
    if len(blinded) != len(evaluated):
        raise ValueError("one evaluated element per blinded element")
    group_size = (len(blinded) or 1) if group_size is None else int(group_size)
    if group_size <= 0 or len(blinded) % group_size:
        raise ValueError("%d elements are not a whole number of groups of %d" % (len(blinded), group_size))
    return blinded, evaluated, group_size, len(blinded) // group_size


def prove(key, blinded, evaluated, dst, group_size=None, nonces=None):
    """The server's proofs (64 bytes each, one per group of `group_size` elements; one group covers everything when None) that
    `evaluated` is evaluate_many(key, blinded).  `nonces`: one int per group, fresh ones from `secrets` when None -- a nonce must be
    uniformly random and must never be used for two proofs."""
    blinded, evaluated, group_size, groups = _groups(blinded, evaluated, group_size)
    nonces = [1 + secrets.randbelow(N - 1) for _ in range(groups)] if nonces is None else [int(r) for r in nonces]
    if len(nonces) != groups:
        raise ValueError("one nonce per group")
    if not groups:
        return []
    eng, comb = _engine_with_comb()
    out, status = eng.dleq_prove(codec.pack_scalars([int(key)])[0], _rows32(blinded), _rows32(evaluated), codec.pack_scalars(nonces), group_size, dst=dst, comb=comb)
    return _checked(out, status, "prove")


def verify(pk, blinded, evaluated, proofs, dst, group_size=None):
    """One bool per group: the proof shows that the group's evaluated elements were made with the key behind `pk`.  An element or a key
    that does not decode, or a proof whose halves are not below N, raises ValueError; a proof that merely does not hold gives False."""
    blinded, evaluated, group_size, groups = _groups(blinded, evaluated, group_size)
    proofs = [bytes(p) for p in proofs]
    if len(proofs) != groups or any(len(p) != 64 for p in proofs):
        raise ValueError("one proof of 64 bytes per group")
    if not groups:
        return []
    eng, comb = _engine_with_comb()
    ok, status = eng.dleq_verify(bytes(pk), _rows32(blinded), _rows32(evaluated), np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(groups, 64), group_size, dst=dst, comb=comb)
    _checked(ok, status, "verify")
    return [bool(v) for v in ok]


def evaluate_direct_many(key, msgs, dst):
    msgs = [bytes(m) for m in msgs]
    if not msgs:
        return []
    matrix, lens = codec.pack_messages(msgs)
    out, status = default_engine().oprf_eval(codec.pack_scalars([int(key)])[0], matrix, lens, dst=dst)
    return _checked(out, status, "evaluate_direct")


def evaluate_direct(key, msg, dst):
    return evaluate_direct_many(key, [msg], dst)[0]
