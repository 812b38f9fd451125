#!/usr/bin/env python3
"""Regenerates tests/golden/dleq.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_dleq.py

The reference has no DLEQ proof; the groups follow the scheme written out in include/fourq_amd.h ("oblivious PRF: proofs").  Hashing is
hashlib's and the map to the curve tests/h2c_ref.py's (itself pinned to the reference's point functions by tests/golden/h2c.json);
everything that is a POINT operation -- the blinding, the server's DH_endo, the composites' multiplications and additions, the nonce's two
multiplications, decode and encode -- is the reference's own MUL_endo, DH_endo, ADD, R1toR2, AffineToR1, R1toAffine, decode and encode
(curve4q.py:405, :467, :174, :109, :100, :103, :49, :41; loaded in memory by oracle/ref_loader.py, nothing of it is copied).  The output
is pure data: per case dst, key, pk and group_size; per group the blinded and evaluated rows, the composite scalars d, M32, Z32 (the
prover's, checked here against the verifier's sum), the nonce and the proof.

DST lengths 1, 2, 69, 70, 129, 130, 197, 198 and 255: where the composite string (110 + |dst| bytes) and the challenge string
(170 + |dst| bytes) cross a SHA-512 block (a string of L bytes takes ceil((L + 17) / 128) blocks: 111 | 112, 239 | 240, 367 | 368).
Group sizes 1, 2, 3 under every DST and one group of 65 (one more than a fold pass takes).  Keys 1, N - 1 and 2^256 - 1 and nonces 1,
N - 1, N + 1 and 2^256 - 1 come first, then random ones.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import h2c_ref  # noqa: E402
import ref_loader  # noqa: E402

N = 0x29CBC14E5E0A72F05397829CBC14E5DFBD004DFE0F79992FB2540EC7768CE7
TOP = (1 << 256) - 1
DST_LENGTHS = [1, 2, 69, 70, 129, 130, 197, 198, 255]
SHAPES = [(1, 2), (2, 2), (3, 1)]                    # (group_size, groups) under every DST
BIG = (65, 1, 70)                                    # group_size, groups, DST length
H2C_DST = b"FourQ-DLEQ-V01-fixture-rows"


def le_mod_n(digest):
    return int.from_bytes(digest, "little") % N


def case(C, rng, dst, key, group_size, groups, nonces):
    mul = lambda m, P: C.R1toAffine(C.MUL_endo(m, C.AffineToR1(P[0], P[1])))
    enc = lambda P: bytes(bytearray(C.encode(P[0], P[1])))
    tail = lambda label: label + dst + bytes([len(dst)])

    def point_sum(scalars, points):
        acc = None
        for k, P in zip(scalars, points):
            T = C.MUL_endo(k, C.AffineToR1(P[0], P[1]))
            acc = T if acc is None else C.ADD(acc, C.R1toR2(T))
        return C.R1toAffine(acc)

    gen = (C.Gx, C.Gy)
    pk32 = enc(C.DH_endo(key, gen))
    K = 392 * key % N
    out = []
    for g in range(groups):
        cpts = [mul(rng.randrange(1, N), h2c_ref.hash_to_curve_affine(b"row %d of group %d, %d bytes of dst" % (j, g, len(dst)), H2C_DST, h2c_ref.RO)) for j in range(group_size)]
        dpts = [C.DH_endo(key, P) for P in cpts]
        cs, ds = [enc(P) for P in cpts], [enc(P) for P in dpts]
        assert all(tuple(C.decode(bytearray(b))) == tuple(P) for b, P in zip(cs + ds, cpts + dpts))
        d = [le_mod_n(hashlib.sha512(pk32 + c + e + j.to_bytes(4, "big") + tail(b"Composite")).digest()) for j, (c, e) in enumerate(zip(cs, ds))]
        M = point_sum(d, cpts)
        Z = C.DH_endo(key, M)
        assert enc(Z) == enc(point_sum(d, dpts))                  # the prover's Z is the verifier's: what the batching rests on
        r = nonces[g] % N
        t2, t3 = enc(mul(r, gen)), enc(mul(r, M))
        c = le_mod_n(hashlib.sha512(pk32 + enc(M) + enc(Z) + t2 + t3 + tail(b"Challenge")).digest())
        s = (r - c * K) % N
        # the verifier's equations, in the reference's own arithmetic
        assert enc(point_sum([s, c], [gen, C.decode(bytearray(pk32))])) == t2 and enc(point_sum([s, c], [M, Z])) == t3
        out.append({"blinded": [b.hex() for b in cs], "evaluated": [b.hex() for b in ds], "d": ["%x" % v for v in d], "M32": enc(M).hex(), "Z32": enc(Z).hex(),
                    "nonce": "%x" % nonces[g], "proof": (c.to_bytes(32, "little") + s.to_bytes(32, "little")).hex()})
    return {"dst": dst.hex(), "key": "%x" % key, "pk": pk32.hex(), "group_size": group_size, "groups": out}


def generate():
    """The text of dleq.json."""
    _, C = ref_loader.load()
    rng = random.Random(20261019)
    keys, nonces = [1, N - 1, TOP], [1, N - 1, N + 1, TOP]
    cases = []
    shapes = [(ln, gs, gr) for ln in DST_LENGTHS for gs, gr in SHAPES] + [(BIG[2], BIG[0], BIG[1])]
    for ln, group_size, groups in shapes:
        dst = bytes(rng.randrange(1, 256) for _ in range(ln))
        key = keys.pop(0) if keys else rng.getrandbits(256)
        rs = [nonces.pop(0) if nonces else rng.getrandbits(256) for _ in range(groups)]
        cases.append(case(C, rng, dst, key, group_size, groups, rs))
    out = {"_layout": "cases of one call each: dst, pk (hex bytes), key (hex integer), group_size, groups; a group: blinded and evaluated rows (hex, group_size of "
                      "each), d (hex integers, the composite scalars), M32, Z32, nonce (hex integer, used mod N), proof = LE32(c) || LE32(s); "
                      "the scheme: include/fourq_amd.h, 'oblivious PRF: proofs'", "cases": cases}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "dleq.json")
    text = generate()
    with open(path, "w") as fh:
        fh.write(text)
    data = json.loads(text)["cases"]
    print("dleq.json %d cases, %d groups, %d bytes" % (len(data), sum(len(c["groups"]) for c in data), len(text)))


if __name__ == "__main__":
    main()
