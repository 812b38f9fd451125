#!/usr/bin/env python3
"""Regenerates tests/golden/msm.json by running the REAL reference (build container only).

    python tests/golden/make_msm.py

Needs the reference (loaded in memory by oracle/ref_loader.py, as make_golden.py does; nothing of it is copied).  The output is pure
data: a dozen groups of 1, 2, 3, 5 or 8 elements, and for every group its scalars k, its affine points P with their encodings, the affine
sum R = R1toAffine(MUL_endo(k_0, P_0) + MUL_endo(k_1, P_1) + ...) and encode(R); integers as hex strings.  Every P is [t]G for the t
recorded beside it, so that a test can check R by the group law as well.

The reference has no multi-scalar function; the expectation is a left-to-right chain of its own ADD over its own MUL_endo, R1toR2,
R1toAffine and encode (curve4q.py:174, :405, :109, :103, :41).  Every point is [t]G with t != 0, so every encoding decodes.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_loader  # noqa: E402

TOP = (1 << 256) - 1


def hx(v):
    if isinstance(v, str):
        return v
    if isinstance(v, int):
        return "%x" % v
    return [hx(e) for e in v]


def generate():
    F, C = ref_loader.load()
    N = C.N
    G1 = C.AffineToR1(C.Gx, C.Gy)
    p = (1 << 127) - 1
    rng = random.Random(20261018)
    rand = lambda: rng.getrandbits(256)

    def point():                                               # (t, [t]G): the tests check the sums by the group law as well
        t = rand() % (N - 1) + 1
        return t, C.R1toAffine(C.MUL_endo(t, G1))

    def neg(tP):
        t, P = tP
        return N - t, (((-P[0][0]) % p, (-P[0][1]) % p), P[1])

    def enc_hex(P):
        return "".join("%02x" % b for b in bytearray(C.encode(P[0], P[1])))

    def group(label, ks, tPs):
        ts, Ps = [t for t, _ in tPs], [P for _, P in tPs]
        assert len(ks) == len(Ps) and all(C.PointOnCurve(P) for P in Ps)
        acc = C.MUL_endo(ks[0], C.AffineToR1(*Ps[0]))
        for k, P in zip(ks[1:], Ps[1:]):
            acc = C.ADD(acc, C.R1toR2(C.MUL_endo(k, C.AffineToR1(*P))))
        R = C.R1toAffine(acc)
        encs = [enc_hex(P) for P in Ps]
        for e, P in zip(encs, Ps):
            assert tuple(C.decode(bytearray.fromhex(e))) == P
        return {"_label": label, "group_size": hx(len(ks)), "k": hx(ks), "t": hx(ts), "P": hx(Ps), "P_enc": encs, "R": hx(R), "R_enc": enc_hex(R)}

    groups = []
    for size in (1, 2, 3, 5, 8):
        groups.append(group("random", [rand() for _ in range(size)], [point() for _ in range(size)]))
    groups.append(group("scalar 0 alone (neutral result)", [0], [point()]))
    k, P = rand(), point()
    groups.append(group("P and -P under the same scalar (sum neutral)", [k, k], [P, neg(P)]))
    k, P = rand(), point()
    groups.append(group("the same point twice (doubling)", [k, k], [P, P]))
    groups.append(group("scalars 0, 1, N", [0, 1, N], [point() for _ in range(3)]))
    groups.append(group("scalars 0, 1, N, 2^256 - 1 and a random one", [0, 1, N, TOP, rand()], [point() for _ in range(5)]))
    groups.append(group("all scalars zero (neutral result)", [0] * 5, [point() for _ in range(5)]))
    k, k2, P, Q = rand(), rand(), point(), point()
    groups.append(group("P and -P at the ends, a point twice in the middle, edge scalars",
                        [k, TOP, k2, k2, N, 1, 0, k], [P, point(), Q, Q, point(), point(), point(), neg(P)]))
    k, P = rand(), point()
    groups.append(group("one point eight times under one scalar", [k] * 8, [P] * 8))
    assert sorted({int(g["group_size"], 16) for g in groups}) == [1, 2, 3, 5, 8]
    out = {"_layout": "per group: k scalars; P = [t]G affine points ((x0, x1), (y0, y1)); P_enc their encode() as hex; R the affine sum "
                      "R1toAffine(MUL_endo(k_0, P_0) + MUL_endo(k_1, P_1) + ...) by a left-to-right chain of the reference's ADD; R_enc = encode(R)",
           "groups": groups}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    text = generate()
    path = os.path.join(HERE, "msm.json")
    with open(path, "w") as fh:
        fh.write(text)
    print("msm.json %d groups, %d bytes" % (len(json.loads(text)["groups"]), len(text)))


if __name__ == "__main__":
    main()
