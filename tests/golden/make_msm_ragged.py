#!/usr/bin/env python3
"""Regenerates tests/golden/msm_ragged.json by running the REAL reference (build container only).

    python tests/golden/make_msm_ragged.py

Needs the reference (loaded in memory by oracle/ref_loader.py, as make_msm.py does; nothing of it is copied).  The output is pure data:
ONE ragged shape -- group lengths 0, 1, 3, 0, 0, 2, 5, 0, 66: empty groups first, adjacent, in the middle and last but one, and a group
longer than the fold factor -- with, per row, the scalar k, the point P = [t]G (t recorded beside it) and its encoding, and per group the
affine sum R = R1toAffine(MUL_endo(k_0, P_0) + MUL_endo(k_1, P_1) + ...) by a left-to-right chain of the reference's own ADD over its own
MUL_endo, R1toR2, R1toAffine and encode, as in make_msm.py.  The sum over NO rows is the neutral the chain would start from: the
reference's R1toAffine of the point (0, 1), and its encode of that.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_loader  # noqa: E402

LENGTHS = [0, 1, 3, 0, 0, 2, 5, 0, 66]
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
    rng = random.Random(20261020)
    rand = lambda: rng.getrandbits(256)

    def enc_hex(P):
        return "".join("%02x" % b for b in bytearray(C.encode(P[0], P[1])))

    neutral = C.R1toAffine(C.AffineToR1((0, 0), (1, 0)))
    edge = iter([0, 1, N - 1, N, N + 1, TOP, TOP, 0])
    groups = []
    for n in LENGTHS:
        ks = [rand() for _ in range(n)]
        if n >= 2:
            ks[0], ks[-1] = next(edge), next(edge)                  # the edge scalars at the first and last row of the groups that have both
        ts = [rand() % (N - 1) + 1 for _ in range(n)]
        Ps = [C.R1toAffine(C.MUL_endo(t, G1)) for t in ts]
        if n:
            acc = C.MUL_endo(ks[0], C.AffineToR1(*Ps[0]))
            for k, P in zip(ks[1:], Ps[1:]):
                acc = C.ADD(acc, C.R1toR2(C.MUL_endo(k, C.AffineToR1(*P))))
            R = C.R1toAffine(acc)
        else:
            R = neutral
        encs = [enc_hex(P) for P in Ps]
        for e, P in zip(encs, Ps):
            assert tuple(C.decode(bytearray.fromhex(e))) == P
        groups.append({"length": hx(n), "k": hx(ks), "t": hx(ts), "P": hx(Ps), "P_enc": encs, "R": hx(R), "R_enc": enc_hex(R)})
    out = {"_layout": "one ragged shape, group after group: k scalars; P = [t]G affine points ((x0, x1), (y0, y1)); P_enc their encode() as hex; R the affine "
                      "sum of MUL_endo(k_i, P_i) over the group's rows by a left-to-right chain of the reference's ADD, the neutral (0, 1) for a group "
                      "of no rows; R_enc = encode(R)",
           "lengths": hx(LENGTHS), "groups": groups}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    text = generate()
    with open(os.path.join(HERE, "msm_ragged.json"), "w") as fh:
        fh.write(text)
    print("msm_ragged.json %d groups, %d bytes" % (len(json.loads(text)["groups"]), len(text)))


if __name__ == "__main__":
    main()
