"""Hash to curve on `bytes`, computed on the GPU through the process-wide engine (fourq_hash_to_curve_* of include/fourq_amd.h, where the
construction is written out): RFC 9380 with SHA-512 XMD, Elligator 2 over GF(p^2) and the x392 chain.

    P = hash_to_curve(msg, dst)                  32-byte encoding of the point; mode="nu" for the non-uniform flavour
    Ps = hash_to_curve_many(msgs, dst)           one batched call

The suite names (FourQ_XMD:SHA-512_ELL2_RO_ / _NU_) are this project's own; `dst` is the caller's domain separation tag, 1..255 bytes.
There is no CPU fallback.
"""
from . import codec
from .engine import default_engine

# one fixed input and the point the CPU restatement of the construction (tests/h2c_ref.py) gives for it: data, for the self-tests
KAT_DST = b"QUUX-V01-CS02-with-FourQ_XMD:SHA-512_ELL2_RO_"
KAT_MSG = b"abc"
KAT_POINT = "f0868f2a33ad027dac9b3387d6039532f04246afdf1e11e5805cc4a85c918180"


def hash_to_curve_many(msgs, dst, mode="ro"):
    """List of 32-byte encodings, one per message."""
    msgs = [bytes(m) for m in msgs]
    if not msgs:
        return []
    matrix, lens = codec.pack_messages(msgs)
    return [r.tobytes() for r in default_engine().hash_to_curve(matrix, lens, dst=dst, mode=mode)]


def hash_to_curve(msg, dst, mode="ro"):
    return hash_to_curve_many([msg], dst, mode)[0]
