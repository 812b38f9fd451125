#!/usr/bin/env python3
"""Regenerates tests/golden/keyset_adversarial.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_keyset_adversarial.py

For every key of tests/keyset_adversarial.py -- the families "strings", "shifted" and "structured", in that order -- the status byte
fourq_keyset_set gives its slot (include/fourq_amd.h, "signatures of registered keys"), computed as make_keyset.py computes it: the
reference's own decode, then [N]A by plain double-and-add with its DBL and its complete ADD (curve4q.py:49, :138, :174, :109, :100, :103;
loaded in memory by oracle/ref_loader.py, nothing of it is copied).  The output is pure data: the status bytes as one hex string, the
SHA-256 of the concatenated key bytes (the keys themselves are rebuilt by the helper, not stored) and the per-family counts.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import ref_loader  # noqa: E402
import keyset_adversarial as ka  # noqa: E402

BYTES_DECODE_BASE, KEYSET_NOT_ORDER_N = 16, 96
DECODE_RESERVED_BIT, DECODE_NOT_ON_CURVE, DECODE_REF_ATTRIBUTE_ERROR = 1, 2, 3


def generate():
    """The text of keyset_adversarial.json."""
    _, C = ref_loader.load()
    assert C.N == ka.N
    N = C.N

    def plain_mul(k, P):
        P1 = C.AffineToR1(P[0], P[1])
        P2 = C.R1toR2(P1)
        Q = P1
        for bit in bin(k)[3:]:
            Q = C.DBL(Q)
            if bit == "1":
                Q = C.ADD(Q, P2)
        return C.R1toAffine(Q)

    def decode_status(pk):
        try:
            return 0, C.decode(bytearray(pk))
        except AttributeError:
            return BYTES_DECODE_BASE + DECODE_REF_ATTRIBUTE_ERROR, None
        except Exception as exc:
            return BYTES_DECODE_BASE + (DECODE_NOT_ON_CURVE if "not on curve" in str(exc) else DECODE_RESERVED_BIT), None

    memo = {}

    def key_status(pk):
        if pk not in memo:
            st, A = decode_status(pk)
            if not st:
                Q = plain_mul(N, A)
                st = 0 if [[int(c) for c in coord] for coord in Q] == [[0, 0], [1, 0]] else KEYSET_NOT_ORDER_N
            memo[pk] = st
        return memo[pk]

    keys = ka.all_keys()
    statuses = bytes(key_status(b) for _, _, b in keys)
    counts = {}
    for name, _, _ in keys:
        counts[name] = counts.get(name, 0) + 1
    out = {"_layout": "statuses: one byte per key of keyset_adversarial.all_keys(), in its order, as hex -- the status fourq_keyset_set gives the "
                      "key's slot; keys_sha256: SHA-256 of the keys' 32-byte strings back to back; counts: keys per family, in order",
           "counts": counts, "keys_sha256": ka.keys_sha256(), "statuses": statuses.hex()}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "keyset_adversarial.json")
    text = generate()
    with open(path, "w") as fh:
        fh.write(text)
    data = json.loads(text)
    print("keyset_adversarial.json %s keys, %d bytes" % (data["counts"], len(text)))


if __name__ == "__main__":
    main()
