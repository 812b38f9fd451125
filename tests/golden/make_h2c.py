#!/usr/bin/env python3
"""Regenerates tests/golden/h2c.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_h2c.py

The reference has no hash-to-curve; the rows follow the construction written out in include/fourq_amd.h ("bytes to a point"): hashing and
the Elligator 2 map are those of tests/h2c_ref.py (hashlib, the oracle's field functions), and everything that is a POINT operation --
the membership test of each mapped point, the sum, the x392 chain, the lowering and the encoding -- is the reference's own PointOnCurve,
ADD, DBL, R1toR2, R1toAffine and encode (curve4q.py:23, :174, :138, :109, :103, :41; loaded in memory by oracle/ref_loader.py, nothing of
it is copied).  The output is pure data: dst, msg, mode -> u, the mapped points, the result as affine words and as its 32 bytes.

Message lengths: 0, 1, 15, 16, 17 and, per DST, the lengths around which b_0's padded string (128 + len + 3 + |DST| + 1 bytes, then the
0x80 marker and the 16 length bytes) grows by a 128-byte block: the last length that fits k blocks and its neighbours, for the first two such k; the first
length of a new block count in both modes.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import h2c_ref as ref  # noqa: E402
import ref_loader  # noqa: E402

F, C = ref_loader.load()
DST_LENGTHS = [1, 16, 43, 255]
BASE_LENGTHS = [0, 1, 15, 16, 17]


def boundary_lengths(dst_len):
    """Message lengths around the first two points where the blocks of b_0 behind Z_pad go from k to k + 1 (with a 255-byte DST the empty
    message already takes three blocks)."""
    out, k = [], 1
    while len(out) < 6:
        last = 128 * k - (3 + dst_len + 1) - 17           # the longest message whose string still fits k blocks
        if last >= 1:
            out += [last - 1, last, last + 1]
        k += 1
    return out


def dst_of(n):
    tag = b"QUUX-V01-CS02-with-FourQ_XMD:SHA-512_ELL2_RO_"
    assert len(tag) == 45
    return (tag * 6)[:n] if n != 43 else tag[:43]


def cofactor_392(Q):
    P0 = C.AffineToR1(Q[0], Q[1])
    P2 = C.ADD(C.DBL(P0), C.R1toR2(P0))
    P3 = C.DBL(C.DBL(C.DBL(C.DBL(P2))))
    return C.R1toAffine(C.DBL(C.DBL(C.DBL(C.ADD(P3, C.R1toR2(P0))))))


def row(dst, msg, mode):
    u = ref.hash_to_field(msg, dst, mode)
    Q = [ref.map_to_curve(x) for x in u]
    assert all(C.PointOnCurve(q) for q in Q)
    S = Q[0] if mode == ref.NU else C.R1toAffine(C.ADD(C.AffineToR1(*Q[0]), C.R1toR2(C.AffineToR1(*Q[1]))))
    P = cofactor_392(S)
    assert C.PointOnCurve(P)
    hx = lambda a: ["%x" % a[0], "%x" % a[1]]
    return {"dst": dst.hex(), "msg": msg.hex(), "mode": "ro" if mode == ref.RO else "nu", "u": [hx(x) for x in u], "mapped": [[hx(q[0]), hx(q[1])] for q in Q],
            "affine": [hx(P[0]), hx(P[1])], "point": bytes(bytearray(C.encode(P[0], P[1]))).hex()}


def main():
    rng = random.Random(20261017)
    rand = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    rows = []
    for dl in DST_LENGTHS:
        dst = dst_of(dl)
        for ln in BASE_LENGTHS + boundary_lengths(dl):
            msg, mode = rand(ln), ref.RO if len(rows) % 2 == 0 else ref.NU
            rows.append(row(dst, msg, mode))
            if ln in boundary_lengths(dl)[2::3]:
                rows.append(row(dst, msg, ref.RO + ref.NU - mode))
        rows.append(row(dst, b"abc", ref.RO))
        rows.append(row(dst, b"abc", ref.NU))
    out = {"_layout": "dst, msg (hex), mode -> u = hash_to_field, mapped = map_to_curve(u_i) affine, affine / point = [392](sum); integers as hex; "
                      "the construction: include/fourq_amd.h", "rows": rows}
    path = os.path.join(HERE, "h2c.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("h2c.json %d rows, %d bytes" % (len(rows), os.path.getsize(path)))


if __name__ == "__main__":
    main()
