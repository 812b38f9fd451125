#!/usr/bin/env python3
"""Regenerates tests/golden/schnorrq.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_schnorrq.py

The reference has no signature scheme; the rows follow the scheme written out in include/fourq_amd.h ("signatures from bytes") with the
reference's own MUL_endo, R1toAffine and encode (curve4q.py:405, :103, :41; loaded in memory by oracle/ref_loader.py, nothing of it is
copied) and hashlib's SHA-512.  The output is pure data: sk, msg -> pk, sig as hex strings.  Message lengths sit on the one- to two-block
boundaries of both hashed strings (32 + len and 64 + len against 111 / 112 / 128).  LE(H(sk)[0:32]) is a 256-bit value and N has 246 bits,
so nearly every row has it >= N; two rows with a value below N are searched for.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_loader  # noqa: E402

F, C = ref_loader.load()
N = C.N
G1 = C.AffineToR1(C.Gx, C.Gy)
LENGTHS = [0, 1, 15, 16, 17, 47, 48, 79, 80, 111, 112, 127, 128, 129, 1000]


def H(b):
    return hashlib.sha512(bytes(b)).digest()


def LE(b):
    return int.from_bytes(bytes(b), "little")


def mul_g(m):
    P = C.R1toAffine(C.MUL_endo(m, G1))
    return bytes(bytearray(C.encode(P[0], P[1])))


def row(label, sk, msg):
    k = H(sk)
    a = LE(k[:32])
    pk = mul_g(a)
    r = LE(H(k[32:] + msg)) % N
    R = mul_g(r)
    h = LE(H(R + pk + msg)) % N
    s = (r - a * h) % N
    return {"_label": label, "_a_ge_N": a >= N, "sk": sk.hex(), "msg": msg.hex(), "pk": pk.hex(), "sig": (R + s.to_bytes(32, "little")).hex()}


def main():
    rng = random.Random(20261016)
    rand = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    rows = []
    for ln in LENGTHS:
        for rep in range(2):
            rows.append(row("length %d" % ln, rand(32), rand(ln)))
    while len(rows) < 40:
        rows.append(row("random", rand(32), rand(rng.randrange(0, 200))))
    small = 0
    while small < 2:                                          # LE(k[0:32]) < N happens once in ~1 500 keys: search for two
        sk = rand(32)
        if LE(H(sk)[:32]) < N:
            rows.append(row("a < N", sk, rand(33)))
            small += 1
    rows.append(row("all-zero key, empty message", bytes(32), b""))
    rows.append(row("all-ones key", bytes([255] * 32), b"FourQ"))
    assert sum(1 for r in rows if r["_a_ge_N"]) >= 30
    out = {"_layout": "sk (32 bytes), msg -> pk = encode([LE(H(sk)[0:32])]G), sig = R || s; H = SHA-512; hex strings; the scheme: include/fourq_amd.h",
           "rows": rows}
    path = os.path.join(HERE, "schnorrq.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("schnorrq.json %d rows, %d bytes" % (len(rows), os.path.getsize(path)))


if __name__ == "__main__":
    main()
