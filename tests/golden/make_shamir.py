#!/usr/bin/env python3
"""Regenerates tests/golden/shamir.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_shamir.py

The reference has no secret sharing; the rows follow include/fourq_amd.h ("threshold sharing").  The scalar side is Python integers;
everything that is a POINT operation -- the commitments [a_j]G, the verification shares sum [x^j]C_j, the points [s_i]P of the combine in
the exponent and their combination -- is the reference's own MUL_endo, ADD, R1toR2, AffineToR1, R1toAffine, decode and encode (loaded in
memory by oracle/ref_loader.py, nothing of it is copied).  The output is pure data.

Polynomials with t in {1, 2, 3, 5} whose coefficients mix random values with the edges 1, N - 1, N + 1 and 2^256 - 1; their commitments;
their shares and verification shares at the ids 1, 2, 7 and 2^32 - 1; the Lagrange coefficients of three id sets; and one combination in
the exponent: three of five parties' points [s_i]P giving [f(0)]P.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_loader  # noqa: E402

N = 0x29CBC14E5E0A72F05397829CBC14E5DFBD004DFE0F79992FB2540EC7768CE7
IDS = [1, 2, 7, (1 << 32) - 1]
THRESHOLDS = [1, 2, 3, 5]
SETS = [[1, 2, 7], [(1 << 32) - 1, 1], [2, 7, 1, (1 << 32) - 1, 5]]
H = lambda v: "%064x" % v


def horner(poly, x):
    acc = 0
    for a in reversed(poly):
        acc = (acc * x + a) % N
    return acc


def lagrange(ids):
    out = []
    for i, xi in enumerate(ids):
        num = den = 1
        for j, xj in enumerate(ids):
            if j != i:
                num, den = num * xj % N, den * (xj - xi) % N
        out.append(num * pow(den, -1, N) % N)
    return out


def generate():
    """The text of shamir.json."""
    _, C = ref_loader.load()
    rng = random.Random(20261021)
    gen = C.AffineToR1(C.Gx, C.Gy)
    enc = lambda P: bytes(bytearray(C.encode(P[0], P[1]))).hex()
    mul = lambda m, R1: C.MUL_endo(m, R1)

    def point_sum(scalars, encodings):
        acc = None
        for k, b in zip(scalars, encodings):
            P = C.decode(bytearray(bytes.fromhex(b)))
            T = mul(k, C.AffineToR1(P[0], P[1]))
            acc = T if acc is None else C.ADD(acc, C.R1toR2(T))
        return enc(C.R1toAffine(acc))

    edges = [1, N - 1, N + 1, (1 << 256) - 1]
    polys = []
    for t in THRESHOLDS:
        for variant in range(2):
            poly = [rng.randrange(1, 1 << 256) for _ in range(t)]
            if variant:
                poly[rng.randrange(t)] = edges[THRESHOLDS.index(t)]
            commits = [enc(C.R1toAffine(mul(a, gen))) for a in poly]
            shares = [horner(poly, x) for x in IDS]
            public = [point_sum([pow(x, j, N) for j in range(t)], commits) for x in IDS]
            for s, p in zip(shares, public):
                assert p == enc(C.R1toAffine(mul(s, gen)))
            polys.append({"t": t, "coeffs": [H(a) for a in poly], "commits": commits, "shares": [H(s) for s in shares], "public": public})
    sets = [{"ids": ids, "lambda": [H(l) for l in lagrange(ids)]} for ids in SETS]
    # three of five: P a point of order N that is not the generator, the parties' points [s_i]P, the combination [f(0)]P
    poly = [rng.randrange(1, N) for _ in range(3)]
    five = [3, 1, 4, 9, (1 << 32) - 1]
    base = mul(rng.randrange(1, N), gen)
    base = C.AffineToR1(*C.R1toAffine(base))
    pick = [five[4], five[0], five[2]]
    points = [enc(C.R1toAffine(mul(horner(poly, x), base))) for x in pick]
    combined = point_sum(lagrange(pick), points)
    assert combined == enc(C.R1toAffine(mul(poly[0], base)))
    exponent = {"coeffs": [H(a) for a in poly], "base": enc(C.R1toAffine(base)), "ids": pick, "points": points, "combined": combined}
    out = {"_layout": "polys: t, coeffs (hex integers below 2^256, coeffs[0] the secret), commits = encode([a_j]G), shares and public = "
                      "encode([share]G) = encode(sum [id^j]C_j) at the ids of 'ids' in that order; sets: ids and their Lagrange coefficients at 0; "
                      "exponent: three parties' points [f(id)]base and combined = encode(sum [lambda_i]point_i) = encode([f(0)]base); "
                      "the scheme: include/fourq_amd.h, 'threshold sharing'",
           "ids": IDS, "polys": polys, "sets": sets, "exponent": exponent}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "shamir.json")
    text = generate()
    with open(path, "w") as fh:
        fh.write(text)
    print("shamir.json %d polynomials, %d bytes" % (len(json.loads(text)["polys"]), len(text)))


if __name__ == "__main__":
    main()
