"""SchnorrQ-shaped signatures on `bytes`, computed on the GPU through the process-wide engine (fourq_sig_* of include/fourq_amd.h, where
the scheme is written out): SHA-512 and the arithmetic modulo N run on the device, the comb of the generator is built and staged once.

    pk = keygen(sk)                  32-byte secret key -> 32-byte public key
    sig = sign(sk, msg)              64 bytes R || s
    verify(pk, msg, sig)             True / False

`sign_many` / `verify_many` take lists and make one batched call.  Byte-for-byte interoperability with FourQlib's schnorrq.c is not
claimed (include/fourq_amd.h); there is no CPU fallback.
"""
import threading

import numpy as np

from . import codec, constants
from .engine import default_engine

_lock = threading.Lock()
_comb = {}


def _engine():
    """The default engine with the comb of G staged on it (built once per engine)."""
    eng = default_engine()
    with _lock:
        comb = _comb.get(id(eng))
        if comb is None:
            g_r1 = codec.pack_point((constants.Gx, constants.Gy, (1, 0), constants.Gx, constants.Gy))      # AffineToR1(Gx, Gy)
            comb = _comb[id(eng)] = eng.comb_table(g_r1)
    return eng, comb


def _rows(items, width, what):
    items = [bytes(b) for b in items]
    if any(len(b) != width for b in items):
        raise ValueError("%s must be %d bytes" % (what, width))
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), width)


def keygen_many(sks):
    eng, comb = _engine()
    return [r.tobytes() for r in eng.sig_keygen(_rows(sks, 32, "a secret key"), comb)]


def sign_many(sks, msgs, pks=None):
    """One signature per (sk, msg); `pks`: the matching public keys where the caller has them (derived otherwise)."""
    eng, comb = _engine()
    sk = _rows(sks, 32, "a secret key")
    pk = eng.sig_keygen(sk, comb) if pks is None else _rows(pks, 32, "a public key")
    matrix, lens = codec.pack_messages(msgs)
    return [r.tobytes() for r in eng.sig_sign(sk, pk, matrix, lens, comb)]


def verify_many(pks, msgs, sigs):
    """List of bool, one per (pk, msg, sig)."""
    eng, comb = _engine()
    matrix, lens = codec.pack_messages(msgs)
    ok, _ = eng.sig_verify(_rows(pks, 32, "a public key"), matrix, _rows(sigs, 64, "a signature"), lens, comb)
    return [bool(v) for v in ok]


def keygen(sk):
    return keygen_many([sk])[0]


def sign(sk, msg):
    return sign_many([sk], [msg])[0]


def verify(pk, msg, sig):
    return verify_many([pk], [msg], [sig])[0]
