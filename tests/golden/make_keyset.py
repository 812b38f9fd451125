#!/usr/bin/env python3
"""Regenerates tests/golden/keyset.json by running the REAL reference's point functions (build container only).

    python tests/golden/make_keyset.py

The reference has neither a signature scheme nor a key set; the rows follow include/fourq_amd.h ("signatures from bytes", "signatures of
registered keys") with the reference's own MUL_endo, DBL, ADD, R1toR2, AffineToR1, R1toAffine, encode and decode (curve4q.py:405, :138,
:174, :109, :100, :103, :41, :49; loaded in memory by oracle/ref_loader.py, nothing of it is copied) and hashlib's SHA-512.  The output is
pure data.

Keys: three honest ones, one that does not decode (an off-curve string of tests/golden/wire.json), and (-x, -y) of the first honest key --
A + (0, -1), a point of order 2N that decodes.  The order check is [N]A by plain double-and-add with DBL and the complete ADD.
Signature rows: per honest key a valid row and the row-level tamper classes of tests/test_sig_oracle.TAMPERS; the key-level classes become
rows that name another key, the refused ones included; s = N exactly; s + N under a refused key (the key's status wins).
Scalar rows: the cross product of {0, 1, 2, N - 1, N, N + 1, 2^256 - 1} for k and l -- all four parity combinations, so all four
combinations of the comb's two even-scalar negations -- over the honest keys, and one row per refused key.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_loader  # noqa: E402

P127 = (1 << 127) - 1
BYTES_DECODE_BASE, SIG_S_RANGE, KEYSET_NOT_ORDER_N = 16, 32, 96
DECODE_RESERVED_BIT, DECODE_NOT_ON_CURVE, DECODE_REF_ATTRIBUTE_ERROR = 1, 2, 3
TOP = (1 << 256) - 1


def H(b):
    return hashlib.sha512(bytes(b)).digest()


def LE(b):
    return int.from_bytes(bytes(b), "little")


def generate():
    """The text of keyset.json."""
    _, C = ref_loader.load()
    N = C.N
    G1 = C.AffineToR1(C.Gx, C.Gy)
    rng = random.Random(20261021)
    rand = lambda n: bytes(rng.getrandbits(8) for _ in range(n))

    def enc(P):
        return bytes(bytearray(C.encode(P[0], P[1])))

    def mul_g(m):
        return enc(C.R1toAffine(C.MUL_endo(m, G1)))

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

    def key_status(pk):
        st, A = decode_status(pk)
        if st:
            return st
        Q = plain_mul(N, A)
        return 0 if [[int(c) for c in coord] for coord in Q] == [[0, 0], [1, 0]] else KEYSET_NOT_ORDER_N

    sks = [rand(32) for _ in range(3)]
    keys = [mul_g(LE(H(sk)[:32])) for sk in sks]
    with open(os.path.join(HERE, "wire.json")) as fh:
        keys.append([bytes.fromhex(r[0]) for r in json.load(fh)["strings"] if r[1] == "Exception" and "not on curve" in r[2]][0])
    x, y = C.decode(bytearray(keys[0]))
    neg = lambda a: ((P127 - int(a[0])) % P127, (P127 - int(a[1])) % P127)
    keys.append(enc((neg(x), neg(y))))
    statuses = [key_status(pk) for pk in keys]
    assert statuses == [0, 0, 0, BYTES_DECODE_BASE + DECODE_NOT_ON_CURVE, KEYSET_NOT_ORDER_N], statuses
    assert C.PointOnCurve(C.decode(bytearray(keys[4])))

    def sign(j, msg):
        k = H(sks[j])
        a = LE(k[:32])
        r = LE(H(k[32:] + msg)) % N
        R = mul_g(r)
        h = LE(H(R + keys[j] + msg)) % N
        return R + ((r - a * h) % N).to_bytes(32, "little")

    def verify(kid, msg, sig):
        if statuses[kid]:
            return 0, statuses[kid]
        s = LE(sig[32:])
        if s >= N:
            return 0, SIG_S_RANGE
        h = LE(H(sig[:32] + keys[kid] + msg)) % N
        A = C.decode(bytearray(keys[kid]))
        Pt = C.ADD(C.MUL_endo(s, G1), C.R1toR2(C.MUL_endo(h, C.AffineToR1(A[0], A[1]))))
        return (1 if enc(C.R1toAffine(Pt)) == sig[:32] else 0), 0

    rows = []

    def row(how, kid, msg, sig):
        ok, st = verify(kid, msg, sig)
        rows.append({"_how": how, "id": kid, "msg": msg.hex(), "sig": sig.hex(), "ok": ok, "status": st})

    for j in range(3):
        msg = rand((33, 112, 5)[j])
        sig = sign(j, msg)
        row("valid", j, msg, sig)
        m = bytearray(msg); m[len(m) // 2] ^= 4
        row("msg bit", j, bytes(m), sig)
        t = bytearray(sig); t[7] ^= 1
        row("R bit", j, msg, bytes(t))
        t = bytearray(sig); t[32 + 3] ^= 8
        row("s bit", j, msg, bytes(t))
        t = bytearray(sig); t[32:] = (LE(sig[32:]) + N).to_bytes(32, "little")
        row("s + N", j, msg, bytes(t))
        row("length one short", j, msg[:-1], sig)
        row("pk bit: another honest key", (j + 1) % 3, msg, sig)
    msg = rand(40)
    sig = sign(0, msg)
    row("s = N", 0, msg, sig[:32] + N.to_bytes(32, "little"))
    row("pk off curve: a key that does not decode", 3, msg, sig)
    row("pk of order 2N", 4, msg, sig)
    row("s + N under a key that does not decode", 3, msg, sig[:32] + (LE(sig[32:]) + N).to_bytes(32, "little"))
    row("s + N under a key of order 2N", 4, msg, sig[:32] + (LE(sig[32:]) + N).to_bytes(32, "little"))
    assert [r["ok"] for r in rows if r["_how"] == "valid"] == [1, 1, 1] and sum(r["ok"] for r in rows) == 3
    assert {r["status"] for r in rows} == {0, SIG_S_RANGE, statuses[3], statuses[4]}

    edges = [0, 1, 2, N - 1, N, N + 1, TOP]
    scalar_rows = []

    def scalar_row(kid, k, l):
        if statuses[kid]:
            out, st = bytes(32), statuses[kid]
        else:
            A = C.decode(bytearray(keys[kid]))
            Pt = C.ADD(C.MUL_endo(k, G1), C.R1toR2(C.MUL_endo(l, C.AffineToR1(A[0], A[1]))))
            out, st = enc(C.R1toAffine(Pt)), 0
        scalar_rows.append({"id": kid, "k": "%x" % k, "l": "%x" % l, "out": out.hex(), "status": st})

    for a, k in enumerate(edges):
        for b, l in enumerate(edges):
            scalar_row((a + b) % 3, k, l)
    scalar_row(3, 5, 7)
    scalar_row(4, 5, 7)
    assert scalar_rows[0]["out"] == "01" + "00" * 31                                        # k = l = 0: the neutral is an ordinary result
    out = {"_layout": "keys: 32-byte strings as hex with the status fourq_keyset_set gives their slot; rows: id, msg, sig (hex bytes) -> ok, status "
                      "of the keyed verify; scalar_rows: id, k, l (hex integers, used as they are) -> out (32 hex bytes) and status of the keyed "
                      "double multiplication",
           "keys": [{"pk": pk.hex(), "status": st} for pk, st in zip(keys, statuses)], "rows": rows, "scalar_rows": scalar_rows}
    return json.dumps(out, separators=(",", ":")) + "\n"


def main():
    path = os.path.join(HERE, "keyset.json")
    text = generate()
    with open(path, "w") as fh:
        fh.write(text)
    data = json.loads(text)
    print("keyset.json %d keys, %d rows, %d scalar rows, %d bytes" % (len(data["keys"]), len(data["rows"]), len(data["scalar_rows"]), len(text)))


if __name__ == "__main__":
    main()
