#!/usr/bin/env python3
"""Regenerates tests/golden/vrf.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_vrf.py

The reference has no VRF; the rows follow the scheme written out in include/fourq_amd.h ("verifiable random function").  Hashing is
hashlib's and the map to the curve tests/h2c_ref.py's (itself pinned to the reference's point functions by tests/golden/h2c.json);
everything that is a POINT operation -- the key, Gamma, the nonce's two multiplications, the x392 chain, the verifier's two sums, decode
and encode -- is the reference's own MUL_endo, DBL, ADD, R1toR2, AffineToR1, R1toAffine, decode and encode (loaded in memory by
oracle/ref_loader.py, nothing of it is copied).  The output is pure data: per row dst, sk, pk, alpha, h32, the proof and beta.

DST lengths 1 and 255; alpha lengths 0, 1, 31, 32, 33, 95, 96 and 97 under both, so that the end of Z_pad || pk32 || alpha || ... lands on
either side of a SHA-512 block and of its padding boundary; two rows of 200 bytes under a DST of 70; and, under both DST lengths, proofs
whose Gamma a dishonest prover has shifted by a point of order 7 and of order 14 (tests/adversarial_points.torsion()) before hashing the
challenge: the verifier's equations hold for them, and beta is the honest row's.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import adversarial_points  # noqa: E402
import h2c_ref  # noqa: E402
import ref_loader  # noqa: E402

N = 0x29CBC14E5E0A72F05397829CBC14E5DFBD004DFE0F79992FB2540EC7768CE7
INV392 = pow(392, -1, N)
ALPHA_LENGTHS = [0, 1, 31, 32, 33, 95, 96, 97]
DST_LENGTHS = [1, 255]
LONG = (70, 200, 2)                                   # DST length, alpha length, rows
SHIFT_ORDERS = [7, 14]

H = lambda b: hashlib.sha512(b).digest()
LE = lambda b: int.from_bytes(b, "little")


def row(C, sk, alpha, dst, shift=None):
    mul = lambda m, P: C.R1toAffine(C.MUL_endo(m, C.AffineToR1(P[0], P[1])))
    enc = lambda P: bytes(bytearray(C.encode(P[0], P[1])))
    add = lambda A, B: C.R1toAffine(C.ADD(C.AffineToR1(A[0], A[1]), C.R1toR2(C.AffineToR1(B[0], B[1]))))
    tail = lambda label: label + dst + bytes([len(dst)])

    def point_sum(scalars, points):
        acc = None
        for k, P in zip(scalars, points):
            T = C.MUL_endo(k, C.AffineToR1(P[0], P[1]))
            acc = T if acc is None else C.ADD(acc, C.R1toR2(T))
        return C.R1toAffine(acc)

    def times_392(P):                                 # the chain of curve4q.py:450-455
        P1 = C.AffineToR1(P[0], P[1])
        T = C.R1toR2(P1)
        Q = C.ADD(C.DBL(P1), T)
        for _ in range(4):
            Q = C.DBL(Q)
        Q = C.ADD(Q, T)
        for _ in range(3):
            Q = C.DBL(Q)
        return C.R1toAffine(Q)

    gen = (C.Gx, C.Gy)
    k = H(sk)
    x = LE(k[:32])
    pk = enc(mul(x, gen))
    Hpt = h2c_ref.hash_to_curve_affine(pk + alpha, dst, h2c_ref.RO)
    h32 = enc(Hpt)
    r = LE(H(k[32:] + h32)) % N
    honest = mul(x, Hpt)
    Gamma = honest if shift is None else add(honest, shift)
    gamma32 = enc(Gamma)
    assert tuple(C.decode(bytearray(gamma32))) == tuple(Gamma)
    u32, v32 = enc(mul(r, gen)), enc(mul(r, Hpt))
    c = LE(H(pk + h32 + gamma32 + u32 + v32 + tail(b"VrfVerify"))) % N
    s = (r - c * x) % N
    # the verifier's equations, in the reference's own arithmetic: W is the honest one whatever the shift
    W = times_392(Gamma)
    assert enc(W) == enc(times_392(honest)) and enc(W) == enc(mul(392, honest))
    assert enc(point_sum([s, c], [gen, C.decode(bytearray(pk))])) == u32 and enc(point_sum([s, c * INV392 % N], [Hpt, W])) == v32
    beta = H(enc(W) + tail(b"VrfOutput"))
    return {"dst": dst.hex(), "sk": sk.hex(), "pk": pk.hex(), "alpha": alpha.hex(), "h32": h32.hex(), "w32": enc(W).hex(),
            "proof": (gamma32 + c.to_bytes(32, "little") + s.to_bytes(32, "little")).hex(), "beta": beta.hex()}


def generate():
    """The text of vrf.json."""
    _, C = ref_loader.load()
    rng = random.Random(20261020)
    rand = lambda n: bytes(rng.randrange(256) for _ in range(n))
    rows = []
    dsts = {ln: bytes(rng.randrange(1, 256) for _ in range(ln)) for ln in DST_LENGTHS + [LONG[0]]}
    for ln in DST_LENGTHS:
        for al in ALPHA_LENGTHS:
            rows.append(dict(row(C, rand(32), rand(al), dsts[ln]), kind="honest"))
    for _ in range(LONG[2]):
        rows.append(dict(row(C, rand(32), rand(LONG[1]), dsts[LONG[0]]), kind="honest"))
    torsion = {}
    for label, T in adversarial_points.torsion():
        order = adversarial_points.order_in_392(T) if label.startswith("seeded torsion") else 0
        if order in SHIFT_ORDERS and order not in torsion:
            torsion[order] = T
    for ln in DST_LENGTHS:
        for order in SHIFT_ORDERS:
            sk, alpha = rand(32), rand(40)
            honest = row(C, sk, alpha, dsts[ln])
            shifted = row(C, sk, alpha, dsts[ln], shift=torsion[order])
            assert shifted["beta"] == honest["beta"] and shifted["proof"] != honest["proof"]
            rows.append(dict(shifted, kind="gamma shifted by a point of order %d" % order, honest_proof=honest["proof"]))
    out = {"_layout": "rows of one (key, alpha) each: dst, sk, pk, alpha, h32 = encode(Hpt), w32 = encode([392]Gamma), proof = gamma32 || LE32(c) || LE32(s), "
                      "beta (all hex bytes); kind: honest, or the order of the torsion point a dishonest prover added to Gamma (honest_proof: the same "
                      "row's honest proof; beta is the same); the scheme: include/fourq_amd.h, 'verifiable random function'", "rows": rows}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "vrf.json")
    text = generate()
    with open(path, "w") as fh:
        fh.write(text)
    print("vrf.json %d rows, %d bytes" % (len(json.loads(text)["rows"]), len(text)))


if __name__ == "__main__":
    main()
