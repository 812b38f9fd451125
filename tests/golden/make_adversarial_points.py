#!/usr/bin/env python3
"""Regenerates tests/golden/adversarial_points.json by running the REAL reference (build container only).

    python tests/golden/make_adversarial_points.py

Needs the reference (loaded in memory by oracle/ref_loader.py, as make_golden.py does; nothing of it is copied).  The output is pure
data: for the members of the families of tests/adversarial_points.py, what the reference computes -- encode of every point, the outcome
of decode of every string, the outcomes of DH_endo and DH_windowed on the rows of adversarial_points.dh_rows(), and both MUL_* on the
preimages.  A row does not repeat its member: row i of a family belongs to the i-th member of that family.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import ref_loader  # noqa: E402
import adversarial_points as adv  # noqa: E402

LAYOUT = {
    "_outcomes": "the exceptions the reference raised, [type name, message], in the order they first appeared; \"!k\" below names entry k",
    "members": "per family of adversarial_points.families(), one row per member in its order.  A point: [encode(x, y) as 64 hex digits, "
               "outcome of decode of that string].  A string: the outcome of decode alone.  An outcome is \"!k\", or \"=\" (decode "
               "returned the member itself), or the point decode returned as x0 x1 y0 y1, 32 hex digits each",
    "dh": "one row per row of adversarial_points.dh_rows(): the outcomes of encode(DH_endo(m, decode(B))) and encode(DH_windowed(m, "
          "decode(B))), each \"!k\" or 64 hex digits",
    "preimages_mul": "one row per preimage (label, P, m, S): R1toAffine(MUL_windowed(m, P)) and R1toAffine(MUL_endo(m, P)) as x0 x1 y0 y1",
}


def point_hex(pt):
    return "".join("%032x" % c for coord in pt for c in coord)


def generate():
    F, C = ref_loader.load()
    assert C.N == adv.N
    seen = []

    def failure(exc):
        key = [type(exc).__name__, str(exc)]
        if key not in seen:
            seen.append(key)
        return "!%d" % seen.index(key)

    def decode(b, member=None):
        try:
            pt = C.decode(bytearray(b))
        except Exception as exc:                                   # the reference signals every failure by an exception
            return failure(exc)
        return "=" if pt == member else point_hex(pt)

    members = {}
    for name, fam in adv.families().items():
        rows = []
        for label, v in fam:
            if isinstance(v, bytes):
                rows.append(decode(v))
            else:
                assert C.PointOnCurve(v), label
                enc = bytes(bytearray(C.encode(v[0], v[1])))
                rows.append([enc.hex(), decode(enc, v)])
        members[name] = rows
    dh = []
    for name, label, b, m in adv.dh_rows():
        row = []
        for fn in (C.DH_endo, C.DH_windowed):
            try:
                q = fn(m, C.decode(bytearray(b)))
                row.append(bytes(bytearray(C.encode(q[0], q[1]))).hex())
            except Exception as exc:
                row.append(failure(exc))
        dh.append(row)
    mul = []
    for label, p, m, s in adv.preimages():
        r1 = C.AffineToR1(p[0], p[1])
        mul.append([point_hex(C.R1toAffine(C.MUL_windowed(m, r1))), point_hex(C.R1toAffine(C.MUL_endo(m, r1)))])
    return json.dumps({"_layout": LAYOUT, "_outcomes": seen, "members": members, "dh": dh, "preimages_mul": mul}, separators=(",", ":")) + "\n"


def main():
    out = generate()
    path = os.path.join(HERE, "adversarial_points.json")
    with open(path, "w") as fh:
        fh.write(out)
    print("adversarial_points.json %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
