#!/usr/bin/env python3
"""Regenerates tests/golden/oprf.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_oprf.py

The reference has no oblivious PRF; the rows follow the construction written out in include/fourq_amd.h ("oblivious PRF").  Hashing is
hashlib's and the map to the curve tests/h2c_ref.py's (itself pinned to the reference's point functions by tests/golden/h2c.json);
everything that is a POINT operation -- the blinding and unblinding multiplications, the server's DH_endo, decode and encode -- is the
reference's own MUL_endo, DH_endo, AffineToR1, R1toAffine, decode and encode (curve4q.py:405, :467, :100, :103, :49, :41; loaded in memory
by oracle/ref_loader.py, nothing of it is copied), and 1 / r mod N is Python's pow.  The output is pure data:
dst, msg, r, key -> blinded, evaluated, unblinded (32 bytes each) and output (64 bytes).

Message lengths: 0 and, per DST, both sides of the two edges of F's string E || msg || "Finalize" || dst || len(dst) -- 32 + len + tail
bytes with tail = 8 + |dst| + 1 -- inside a 128-byte block: where the 0x80 marker and the 16 length bytes stop fitting (111 -> 112 bytes
mod 128) and where the string itself fills the block (127, 128, 129).  Blinds 1, N - 1, N + 1 and 2^256 - 1, keys 1, N - 1 and 2^256 - 1,
then random ones; two DSTs, of 1 and of 255 bytes.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import hashlib  # noqa: E402

import h2c_ref  # noqa: E402
import ref_loader  # noqa: E402

N = 0x29CBC14E5E0A72F05397829CBC14E5DFBD004DFE0F79992FB2540EC7768CE7
TOP = (1 << 256) - 1
DSTS = [b"Q", (b"QUUX-V01-CS02-with-FourQ_XMD:SHA-512_ELL2_RO_" * 6)[:255]]


def edge_lengths(dst_len):
    tail = 8 + dst_len + 1
    first = next(k for k in range(1, 8) if 128 * k - 17 - 32 - tail >= 1)
    fits = 128 * first - 17 - 32 - tail               # the longest message whose string, marker and length still fit `first` blocks
    full = 128 * first - 32 - tail                    # the message with which the string alone fills them
    return [fits - 1, fits, fits + 1, full - 1, full, full + 1]


def row(C, dst, msg, r, key):
    A = h2c_ref.hash_to_curve_affine(msg, dst, h2c_ref.RO)
    assert C.PointOnCurve(A)
    mul = lambda m, P: C.R1toAffine(C.MUL_endo(m, C.AffineToR1(P[0], P[1])))
    enc = lambda P: bytes(bytearray(C.encode(P[0], P[1])))
    blinded = enc(mul(r, A))
    evaluated = enc(C.DH_endo(key, C.decode(bytearray(blinded))))
    unblinded = enc(mul(pow(r % N, -1, N), C.decode(bytearray(evaluated))))
    assert unblinded == enc(C.DH_endo(key, A))        # the identity the protocol rests on, in the reference's own arithmetic
    out = hashlib.sha512(unblinded + msg + b"Finalize" + dst + bytes([len(dst)])).digest()
    return {"dst": dst.hex(), "msg": msg.hex(), "r": "%x" % r, "key": "%x" % key, "blinded": blinded.hex(), "evaluated": evaluated.hex(),
            "unblinded": unblinded.hex(), "output": out.hex()}


def generate():
    """The text of oprf.json."""
    _, C = ref_loader.load()
    rng = random.Random(20261019)
    rand = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    blinds, keys = [1, N - 1, N + 1, TOP], [1, N - 1, TOP]
    rows = []
    for dst in DSTS:
        for ln in [0] + edge_lengths(len(dst)):
            i = len(rows)
            r = blinds[i] if i < len(blinds) else rng.getrandbits(256)
            key = keys[i] if i < len(keys) else rng.getrandbits(256)
            rows.append(row(C, dst, rand(ln), r, key))
    rows.append(row(C, DSTS[0], b"abc", rng.randrange(1, N), rng.randrange(1, N)))
    rows.append(row(C, DSTS[1], b"abc", rng.randrange(1, N), rng.randrange(1, N)))
    out = {"_layout": "dst, msg (hex), r, key (hex integers) -> blinded = encode([r]G(msg)), evaluated = encode(DH_endo(key, blinded)), "
                      "unblinded = encode([1 / r mod N]evaluated), output = SHA-512(unblinded || msg || 'Finalize' || dst || len(dst)); "
                      "the construction: include/fourq_amd.h", "rows": rows}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "oprf.json")
    text = generate()
    with open(path, "w") as fh:
        fh.write(text)
    print("oprf.json %d rows, %d bytes" % (len(json.loads(text)["rows"]), len(text)))


if __name__ == "__main__":
    main()
