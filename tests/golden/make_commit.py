#!/usr/bin/env python3
"""Regenerates tests/golden/commit.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_commit.py

The reference has no commitment call; a commitment is out[g] = sum_j [k_gj]B_j as include/fourq_amd.h writes it out ("commitments over a
fixed generator set").  Every point operation -- the bases [t_j]G, the multiplications, the additions, the normalisation and the
encoding -- is the reference's own MUL_endo, ADD, R1toR2, AffineToR1, R1toAffine and encode (curve4q.py:405, :174, :109, :100, :103, :41;
loaded in memory by oracle/ref_loader.py, nothing of it is copied).  The output is pure data: five bases with their t_j, and per case a
group_size, the groups' scalars and the expected affine points and encodings.

Cases: group sizes 1, 2 and 5 with three groups each -- the edge scalars 0, 1, N - 1, N, N + 1 and 2^256 - 1 come first, then random ones --
and one group of five whose last scalar closes the sum: sum_j k_j t_j = 0 (mod N), the neutral point.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_loader  # noqa: E402

N = 0x29CBC14E5E0A72F05397829CBC14E5DFBD004DFE0F79992FB2540EC7768CE7
TOP = (1 << 256) - 1
BASES = 5
SIZES = (1, 2, 5)
GROUPS = 3


def hx(P):
    return [["%x" % c for c in coord] for coord in P]


def generate():
    """The text of commit.json."""
    _, C = ref_loader.load()
    rng = random.Random(20261020)
    G = C.AffineToR1(C.Gx, C.Gy)
    ts = [rng.randrange(2, N) for _ in range(BASES)]
    bases = [tuple(C.R1toAffine(C.MUL_endo(t, G))) for t in ts]

    def commit(ks):
        acc = None
        for k, B in zip(ks, bases):
            T = C.MUL_endo(k, C.AffineToR1(B[0], B[1]))
            acc = T if acc is None else C.ADD(acc, C.R1toR2(T))
        return tuple(C.R1toAffine(acc))

    edges = [0, 1, N - 1, N, N + 1, TOP]
    cases = []
    for size in SIZES:
        groups = []
        for _ in range(GROUPS):
            ks = [edges.pop(0) if edges else rng.getrandbits(256) for _ in range(size)]
            P = commit(ks)
            groups.append({"k": ["%x" % k for k in ks], "affine": hx(P), "enc": bytes(bytearray(C.encode(P[0], P[1]))).hex()})
        cases.append({"group_size": size, "groups": groups})
    ks = [rng.getrandbits(256) for _ in range(BASES - 1)]
    ks.append(-sum(k * t for k, t in zip(ks, ts)) * pow(ts[-1], -1, N) % N)
    P = commit(ks)
    assert [[int(c) for c in coord] for coord in P] == [[0, 0], [1, 0]]
    cases.append({"group_size": BASES, "groups": [{"k": ["%x" % k for k in ks], "affine": hx(P), "enc": bytes(bytearray(C.encode(P[0], P[1]))).hex()}]})
    out = {"_layout": "bases: affine points [[x0, x1], [y0, y1]] (hex integers) with t, B_j = [t_j]G; cases: group_size and groups; a group: its "
                      "group_size scalars k (hex integers, used as they are), the expected affine point and enc, its 32-byte encoding as hex "
                      "BYTES (read it raw); the last case commits to the neutral",
           "t": ["%x" % t for t in ts], "bases": [hx(B) for B in bases], "cases": cases}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "commit.json")
    text = generate()
    with open(path, "w") as fh:
        fh.write(text)
    data = json.loads(text)["cases"]
    print("commit.json %d cases, %d groups, %d bytes" % (len(data), sum(len(c["groups"]) for c in data), len(text)))


if __name__ == "__main__":
    main()
