#!/usr/bin/env python3
"""Regenerates tests/golden/double_mul.json by running the REAL reference (build container only).

    python tests/golden/make_double_mul.py

Needs the reference (loaded in memory by oracle/ref_loader.py, as make_golden.py does; nothing of it is copied).  The output is
pure data: for every case k, l, the affine point P, encode(P), what the reference's decode makes of that encoding, the affine
R = R1toAffine(ADD(MUL_endo(k, G), R1toR2(MUL_endo(l, AffineToR1(P))))) and encode(R); integers as hex strings.

The reference has no double-scalar function; the expectation is composed from its own MUL_endo, R1toR2, ADD, R1toAffine and
encode (curve4q.py:405, :109, :174, :103, :41).  For points outside the order-N subgroup MUL_endo's answer is not [l]P
(the draft says so); the reference's answer is the expectation all the same.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_loader  # noqa: E402

F, C = ref_loader.load()
N = C.N
G = (C.Gx, C.Gy)
G1 = C.AffineToR1(C.Gx, C.Gy)


def hx(v):
    if isinstance(v, str):
        return v
    if isinstance(v, int):
        return "%x" % v
    return [hx(e) for e in v]


def enc_hex(P):
    return "".join("%02x" % b for b in bytearray(C.encode(P[0], P[1])))


def decode_verdict(hexstr):
    """'ok' when the reference decodes the string back to a point, else the exception it raises (type: message)."""
    try:
        C.decode(bytearray.fromhex(hexstr))
        return "ok"
    except Exception as exc:                                   # the reference signals every failure by an exception
        return "%s: %s" % (type(exc).__name__, exc)


def mulG(t):
    return C.R1toAffine(C.MUL_endo(t % N, G1))


def case(label, k, l, P):
    R = C.R1toAffine(C.ADD(C.MUL_endo(k, G1), C.R1toR2(C.MUL_endo(l, C.AffineToR1(P[0], P[1])))))
    e = enc_hex(P)
    return {"_label": label, "k": hx(k), "l": hx(l), "P": hx(P), "P_enc": e, "_P_decode": decode_verdict(e), "R": hx(R), "R_enc": enc_hex(R)}


def main():
    rng = random.Random(20261016)
    kat = json.load(open(os.path.join(HERE, "kat.json")))
    P392 = tuple(tuple(int(c, 16) for c in coord) for coord in kat["P392"])
    off_subgroup = [P392, C.R1toAffine(C.ADD(C.AffineToR1(P392[0], P392[1]), C.R1toR2(G1)))]
    assert all(C.PointOnCurve(Q) for Q in off_subgroup)
    rand = lambda: rng.getrandbits(256)
    cases = []
    for i in range(24):
        cases.append(case("random", rand(), rand(), mulG(rand())))
    edges = [0, 1, N - 1, N, N + 1, (1 << 256) - 1]
    for e in edges:
        cases.append(case("k edge", e, rand(), mulG(rand())))
        cases.append(case("l edge", rand(), e, mulG(rand())))
    for e in (0, N, (1 << 256) - 1):
        cases.append(case("k = l edge", e, e, mulG(rand())))
    cases.append(case("k = l = 0 (neutral result)", 0, 0, mulG(rand())))
    for _ in range(4):                                         # the doubling case of the addition: [k]G == [l]P
        l, t = rand(), rand() % N
        cases.append(case("doubling", (l * t) % N, l, mulG(t)))
    for _ in range(4):                                         # [k]G == -[l]P: the sum is the neutral point
        l, t = rand(), rand() % N
        cases.append(case("sum neutral", (-l * t) % N, l, mulG(t)))
    cases.append(case("doubling, unreduced k", (7 * 11) % N + N, 7, mulG(11)))
    for _ in range(3):
        cases.append(case("P = G", rand(), rand(), G))
    cases.append(case("P = G, k + l = N", 5, N - 5, G))
    for _ in range(3):
        cases.append(case("P neutral", rand(), rand(), (C.Ox, C.Oy)))
    cases.append(case("P neutral, k = 0", 0, rand(), (C.Ox, C.Oy)))
    for Q in off_subgroup:
        for _ in range(3):
            cases.append(case("P outside the order-N subgroup", rand(), rand(), Q))
        cases.append(case("P outside the order-N subgroup, l = 392", rand(), 392, Q))
    out = {"_layout": "k, l: scalars; P, R: affine ((x0, x1), (y0, y1)); P_enc, R_enc: encode() as hex; _P_decode: 'ok' or the "
                      "exception of the reference's decode(P_enc); R = R1toAffine(ADD(MUL_endo(k, G), R1toR2(MUL_endo(l, AffineToR1(P)))))",
           "cases": cases}
    path = os.path.join(HERE, "double_mul.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("double_mul.json %d cases, %d bytes" % (len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
