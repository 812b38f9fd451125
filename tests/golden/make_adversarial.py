#!/usr/bin/env python3
"""Regenerates tests/golden/adversarial.json by running the REAL reference (build container only).

    python tests/golden/make_adversarial.py

Needs the reference (loaded in memory by oracle/ref_loader.py, as make_golden.py does; nothing of it is copied).  The output is
pure data: for the scalars of the three 256-bit families of tests/adversarial_scalars.py, what the reference computes --
decompose(m), recode(decompose(m)), the fixed-window digits of MUL_windowed (re-derived with the reference's own arithmetic, as
make_golden.windowed_digits does: the reference keeps them in local variables) and the affine results of MUL_endo(m, G) and
MUL_windowed(m, G).  Every constructed member is there; the seeded ones follow, in the families' order, while the file stays within
the size of mul.json (the largest fixture of this kind).  A row does not repeat its scalar: row i belongs to the i-th scalar of that order.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import ref_loader  # noqa: E402
import adversarial_scalars as adv  # noqa: E402

LAYOUT = ("rows, one per scalar m in the order given above: decompose(m) as four 16-digit words a1..a4, the 65 sign bits of recode(decompose(m)) as one integer (bit i = "
          "sign i), its 65 digits as a string, the 63 fixed-window digits as one character each ((positive << 3) | (|d| - 1) / 2), "
          "R1toAffine(MUL_endo(m, G)) as four 32-digit words x0 x1 y0 y1, and R1toAffine(MUL_windowed(m, G)) in the same form only "
          "where it differs; integers as hex")
ORDER = ("the constructed members of adversarial_scalars.families256() in its order (labels not starting with 'seeded'), then its seeded "
         "members in its order, as many as fit")


def windowed_digits(C, m):
    red = m % C.N
    if red % 2 == 0:
        red += C.N
    dg = []
    for _ in range(63):
        di = (red % 32) - 16
        dg.append(di)
        red = (red - di) // 16
    dg[62] = red
    return dg


def affine_hex(P):
    return "".join("%032x" % c for coord in P for c in coord)


def row(C, G1, m):
    v = C.decompose(m)
    s, dg = C.recode(v)
    assert len(s) == 65 and len(dg) == 65 and all(0 <= x < (1 << 64) for x in v)
    win = windowed_digits(C, m)
    e, w = C.R1toAffine(C.MUL_endo(m, G1)), C.R1toAffine(C.MUL_windowed(m, G1))
    out = ["".join("%016x" % x for x in v), "%x" % sum(b << i for i, b in enumerate(s)), "".join(map(str, dg)),
           "".join("%x" % ((8 if d > 0 else 0) | ((abs(d) - 1) // 2)) for d in win), affine_hex(e)]
    if w != e:
        out.append(affine_hex(w))
    return out


def generate():
    F, C = ref_loader.load()
    assert C.N == adv.N
    G1 = C.AffineToR1(C.Gx, C.Gy)
    fam = adv.families256()
    rows = [row(C, G1, m) for label, m in fam if not adv.is_seeded(label)]
    limit = os.path.getsize(os.path.join(HERE, "mul.json"))
    text = lambda rs: json.dumps({"_order": ORDER, "_layout": LAYOUT, "rows": rs}, separators=(",", ":")) + "\n"
    for label, m in fam:
        if adv.is_seeded(label):
            more = rows + [row(C, G1, m)]
            if len(text(more)) > limit:
                break
            rows = more
    return text(rows)


def main():
    out = generate()
    path = os.path.join(HERE, "adversarial.json")
    with open(path, "w") as fh:
        fh.write(out)
    print("adversarial.json %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
