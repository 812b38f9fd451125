"""The adversarial point and string families of tests/adversarial_points.py, before any GPU runs (no GPU needed).

1. Every family has the property it is for, shown with plain Python integers: the intermediate values of decode are recomputed here from
   the formulas (curve4q.py:64-75), nothing under fourq_amd/ is imported for them.
2. tests/golden/adversarial_points.json, the real reference's answers, pins oracle/curve4q_oracle.py row by row, and oracle_c.encode on
   every point; where the reference is present the generator must reproduce the file byte for byte.
3. Two models of a wrong device -- a decode whose t == 0 test looks at the integer t0 + t3 instead of its residue, and a sign() without
   its x0 == 0 branch -- are noticed by no random input and by every member built against them (run with -s to see the figures).
4. The mix of outcomes the string families were built for.  No row is skipped anywhere.
"""
import os
import random

import numpy as np
import pytest

import adversarial_points as adv
import curve4q_oracle as o
import oracle_c as oc
import ref_loader
from conftest import GOLDEN, load_golden
from fourq_amd import codec

P = adv.P
FAM = adv.families()
ATTRIBUTE_ERROR = ("AttributeError", "type object 'GFp' has no attribute 'two'")
NOT_ON_CURVE = ("Exception", "Point not on curve")
RESERVED = ("Exception", "Malformed point: reserved bit is not zero")
DH_NEUTRAL = ("Exception", "DH computation resulted in neutral point")


def decode_trace(b):
    """(t0, t1, t3) of decode as integers in [0, p), from y alone (curve4q.py:64-74); Python's pow for the inverse square root"""
    y = (int.from_bytes(b[:16], "little") & P, int.from_bytes(b[16:], "little") & P)
    y2 = o.f2_sqr(y)
    u0, u1 = o.f2_sub(y2, o.F2_ONE)
    v0, v1 = o.f2_add(o.f2_mul(o.d, y2), o.F2_ONE)
    t0 = (u0 * v0 + u1 * v1) % P
    t1 = (u1 * v0 - u0 * v1) % P
    t3 = (t0 * t0 + t1 * t1) % P
    t3 = pow(t3, (1 << 125) - 1, P) * t3 % P
    return t0, t1, t3


# ---- 1. the families have the property they are for -------------------------------------------------------------------------------
def test_every_point_is_on_the_curve_and_the_families_are_deterministic():
    for name, label, pt in adv.on_curve_members():
        assert o.PointOnCurve(pt) and all(0 <= c < P for coord in pt for c in coord), (name, label)
    total = sum(len(v) for v in FAM.values())
    assert 1000 <= total <= 1500, total
    assert {k: v for k, v in FAM.items() if k != "preimages"} == {k: getattr(adv, k)() for k in adv.POINT_FAMILIES + adv.STRING_FAMILIES}
    for name, fam in FAM.items():
        assert len({label for label, _ in fam}) == len(fam) == len({v for _, v in fam}), name


def test_imaginary_x_is_a_zero_that_is_not_the_integer_zero():
    fam = FAM["imaginary_x"]
    assert sum(1 for label, _ in fam if label.startswith("seeded")) == 160 and len(fam) >= 160 + 3
    seen_x1, top = set(), 0
    for label, (x, y) in fam:
        b = adv.encode((x, y))
        assert adv.outcome(b) == ATTRIBUTE_ERROR, label
        if label == "order 2":                                     # y = -1: u = 0, the genuine zero the older tests have
            assert x == (0, 0) and decode_trace(b) == (0, 0, 0)
            continue
        assert x[0] == 0 and x[1] != 0, label
        t0, t1, t3 = decode_trace(b)
        assert t0 != 0 and t0 + t3 == P, label
        assert b[31] >> 7 == x[1] >> 126, label                    # the sign bit comes from x1
        seen_x1.add(x[1])
        top += x[1] >> 126
    with_root = {e for e in adv.E_X if adv.y_from_x((0, e)) is not None}
    assert {1, P - 1} <= with_root <= seen_x1                      # every edge word that has a root, x1 = +-1 among them
    assert sum(1 for v in seen_x1 if abs(v - adv.HALF) < 64) == 4  # and the roots nearest to the sign bit's boundary, both sides
    assert 3 * top >= len(fam)                                     # at least a third has bit 126 of x1 set (half, by construction)
    assert sum(1 for label, (x, y) in fam if y == (0, 0)) == 2     # the two points of order 4


def test_real_x_and_sign_boundary_round_trip():
    assert sum(1 for label, _ in FAM["real_x"] if label.startswith("seeded")) == 80
    for label, pt in FAM["real_x"]:
        b = adv.encode(pt)
        assert pt[0][1] == 0 and adv.outcome(b) == ("ok", pt) and decode_trace(b)[1] == 0, label
    assert {1, P - 1} & {pt[0][0] for _, pt in FAM["real_x"]}
    fam = FAM["sign_boundary"]
    assert len(fam) == 2 * 4 * len(adv.E_X)
    for half in (0, 1):
        for e in adv.E_X:
            assert sum(1 for _, pt in fam if pt[0][half] == e) == 4, (half, e)
    for label, pt in fam:
        assert adv.outcome(adv.encode(pt)) == ("ok", pt), label


def test_torsion_orders_and_dh():
    orders = {}
    dh = {label: (b, m) for name, label, b, m in adv.dh_rows() if name == "torsion"}
    assert len(dh) == len(FAM["torsion"])
    for label, pt in FAM["torsion"]:
        b, m = dh[label]
        if "full order" in label:
            assert adv.scalar_mul(392, pt) != adv.NEUTRAL and adv.scalar_mul(adv.N, pt) != adv.NEUTRAL, label
            assert adv.scalar_mul(adv.ORDER, pt) == adv.NEUTRAL, label
            q = o.DH_endo(m, pt)
            assert q == o.DH_windowed(m, pt) and o.PointOnCurve(q), label
            continue
        n = int(label.split("order ")[1].split(":")[0])
        assert adv.scalar_mul(n, pt) == adv.NEUTRAL, label
        for prime in (2, 7):                                       # exactly n: no proper divisor does
            if n % prime == 0:
                assert adv.scalar_mul(n // prime, pt) != adv.NEUTRAL, label
        orders[n] = orders.get(n, 0) + 1
        for fn in (o.DH_endo, o.DH_windowed):
            with pytest.raises(Exception) as ei:
                fn(m, pt)
            assert (type(ei.value).__name__, str(ei.value)) == DH_NEUTRAL, label
        want = ATTRIBUTE_ERROR if n in (1, 2, 4) else ("ok", pt)   # x0 = 0 for the orders 1, 2 and 4
        assert adv.outcome(adv.encode(pt)) == want, label
    assert all(orders.get(n, 0) >= 3 for n in (7, 14, 28, 56)) and orders[1] == 1 and orders[2] == 1 and orders[4] == 2, orders
    assert sum(1 for label, _ in FAM["torsion"] if "full order" in label) >= 6
    print("\ntorsion orders: %s" % sorted(orders.items()))


def test_subgroup_points_with_a_zero_half_are_what_pipelines_can_emit():
    """the question of whether a pipeline's own output can have x0 = 0: it can.  One point in 392 with x = (0, x1) lies in the subgroup"""
    g1 = o.AffineToR1(o.Gx, o.Gy)
    rows = adv.subgroup_pipelines()
    assert len(rows) == 8 and sum(1 for r in rows if r[1][0][0] == 0) == 4 and sum(1 for r in rows if r[1][0][1] == 0) == 4
    for label, s, m, p, pdh, k, l, pdm in rows:
        assert o.PointOnCurve(s) and adv.scalar_mul(adv.N, s) == adv.NEUTRAL and s != adv.NEUTRAL, label
        for pt in (p, pdh, pdm):
            assert adv.scalar_mul(adv.N, pt) == adv.NEUTRAL and adv.outcome(adv.encode(pt)) == ("ok", pt), label
        r1 = o.AffineToR1(*p)
        assert o.R1toAffine(o.MUL_endo(m, r1)) == s == o.R1toAffine(o.MUL_windowed(m, r1)), label
        assert o.DH_endo(m, pdh) == s == o.DH_windowed(m, pdh), label
        assert o.R1toAffine(o.ADD(o.MUL_endo(k, g1), o.R1toR2(o.MUL_endo(l, o.AffineToR1(*pdm))))) == s, label
        want = ATTRIBUTE_ERROR if s[0][0] == 0 else ("ok", s)
        assert adv.outcome(adv.encode(s)) == want and adv.encode(s)[31] >> 7 == (s[0][1] if s[0][0] == 0 else s[0][0]) >> 126, label


def test_preimages_multiply_back_exactly():
    pre = adv.preimages()
    assert len(pre) == 18 and {m for _, _, m, _ in pre} == set(adv.PREIMAGE_MS)
    zero_half = [0, 0]
    for label, p, m, s in pre:
        assert o.PointOnCurve(p) and adv.outcome(adv.encode(p)) == ("ok", p), label
        r1 = o.AffineToR1(*p)
        assert o.R1toAffine(o.MUL_windowed(m, r1)) == s == adv.scalar_mul(m, p), label
        assert o.MUL_windowed(m, r1)[2] != o.F2_ONE, label        # S arrives with a Z that is not 1
        for half in (0, 1):
            zero_half[half] += s[0][half] == 0
    assert zero_half == [6, 6]


def test_refused_class_is_refused_whatever_lies_underneath():
    fam = dict(FAM["edge_words_y"])
    under = {label: adv.outcome(b) for label, b in fam.items() if label.startswith("underneath")}
    kinds = {("ok" if k == "ok" else k, None if k == "ok" else w) for k, w in under.values()}
    assert kinds == {("ok", None), ATTRIBUTE_ERROR, NOT_ON_CURVE}
    refused = [(label, b) for label, b in fam.items() if label.startswith("refused")]
    assert len(refused) == 2 * (3 + 3 + 5) + 2
    for label, b in refused:
        assert adv.outcome(b) == RESERVED, label
        y0, y1 = int.from_bytes(b[:16], "little"), int.from_bytes(b[16:], "little") & ((1 << 127) - 1)
        assert y0 >> 127 or y0 == P or y1 == P, label
    for which in ("bit 127 of y0", "y0 = p", "y1 = p"):            # each over a t == 0 string and over one off the curve, both sign bits
        for below in ("t == 0", "off the curve"):
            got = [b[31] >> 7 for label, b in refused if which in label and below in label]
            assert {0, 1} <= set(got), (which, below)
    for label, b in fam.items():                                   # bit 127 of y0: the string underneath with that bit cleared is a member
        if "bit 127" in label:
            body = bytearray(b)
            body[15] &= 0x7F
            name = "underneath: " + label.split(" over ")[1].split(", sign")[0]
            assert bytes(body[:31]) == fam[name][:31] and body[31] & 0x7F == fam[name][31] & 0x7F, label


# ---- 2. the fixture ---------------------------------------------------------------------------------------------------------------
def unhex_point(h):
    return tuple((int(h[64 * c:64 * c + 32], 16), int(h[64 * c + 32:64 * c + 64], 16)) for c in range(2))


def fixture():
    g = load_golden("adversarial_points.json", raw=True)
    g["_outcomes"] = [tuple(e) for e in g["_outcomes"]]
    return g


def fixture_outcome(g, cell, member=None):
    if cell.startswith("!"):
        return g["_outcomes"][int(cell[1:])]
    return "ok", (member if cell == "=" else unhex_point(cell))


def test_fixture_pins_the_oracles_row_by_row():
    g = fixture()
    assert list(g["members"]) == list(FAM) and len(g["dh"]) == len(adv.dh_rows()) and len(g["preimages_mul"]) == len(adv.preimages())
    points, encodings = [], []
    for name, fam in FAM.items():
        rows = g["members"][name]
        assert len(rows) == len(fam), name
        for (label, v), row in zip(fam, rows):
            if isinstance(v, bytes):
                assert adv.outcome(v) == fixture_outcome(g, row), (name, label)
            else:
                enc = bytes.fromhex(row[0])
                assert adv.encode(v) == enc, (name, label)
                assert adv.outcome(enc) == fixture_outcome(g, row[1], v), (name, label)
                points.append(v)
                encodings.append(enc)
    got = oc.encode(codec.pack_points(points, 2))                  # the C oracle's encode on every point
    assert [bytes(r) for r in got] == encodings
    for (name, label, b, m), row in zip(adv.dh_rows(), g["dh"]):
        for fn, cell in zip((o.DH_endo, o.DH_windowed), row):
            try:
                got = "ok", adv.encode(fn(m, o.decode(b)))
            except Exception as exc:
                got = type(exc).__name__, str(exc)
            want = g["_outcomes"][int(cell[1:])] if cell.startswith("!") else ("ok", bytes.fromhex(cell))
            assert got == want, (name, label)
    for (label, p, m, s), row in zip(adv.preimages(), g["preimages_mul"]):
        r1 = o.AffineToR1(*p)
        assert o.R1toAffine(o.MUL_windowed(m, r1)) == unhex_point(row[0]) == s, label
        assert o.R1toAffine(o.MUL_endo(m, r1)) == unhex_point(row[1]), label
    assert os.path.getsize(os.path.join(GOLDEN, "adversarial_points.json")) <= os.path.getsize(os.path.join(GOLDEN, "mul.json"))
    sample = [name for name, _, _, _ in adv.dh_rows() if name not in ("torsion", "subgroup_zero_half", "preimages")]
    assert len(sample) == adv.DH_SAMPLE and len(set(sample)) == 5


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_adversarial_points", os.path.join(GOLDEN, "make_adversarial_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "adversarial_points.json")) as fh:
        assert mod.generate() == fh.read()


# ---- 3. what random input does not see ----------------------------------------------------------------------------------------------
def model1_misses(b):
    """a decode whose t == 0 test compares limbs: it sees the integer t0 + t3, which is p here, and goes on"""
    t0, t1, t3 = decode_trace(b)
    return ((t0 + t3) % P == 0) != (t0 + t3 == 0)


def model2_sign(x):
    """sign() without its x0 == 0 branch"""
    return x[0] >> 126


def test_two_wrong_devices_are_noticed_by_the_families_and_by_no_random_input():
    rng = random.Random(9800)
    strings = [adv.y_string(rng.randrange(P), rng.randrange(P), rng.randrange(2)) for _ in range(20000)]
    random_hits = sum(model1_misses(b) for b in strings)
    fam = [(label, pt) for label, pt in FAM["imaginary_x"] if label != "order 2"]
    family_hits = sum(model1_misses(adv.encode(pt)) for _, pt in fam)
    print("\nmodel 1 (t == 0 on the integer t0 + t3): noticed by %d of %d random strings, %d of the %d imaginary_x encodings with y != -1"
          % (random_hits, len(strings), family_hits, len(fam)))
    assert random_hits == 0 and family_hits == len(fam)
    valid = [pt for kind, pt in (adv.outcome(b) for b in strings[:2000]) if kind == "ok"]
    g1 = o.AffineToR1(o.Gx, o.Gy)
    valid += [o.R1toAffine(o.MUL_endo(rng.getrandbits(256), g1)) for _ in range(50)]
    random_hits = sum(model2_sign(pt[0]) != o.sign(pt[0]) for pt in valid)
    top = [(label, pt) for label, pt in FAM["imaginary_x"] if pt[0][1] >> 126]
    family_hits = sum(model2_sign(pt[0]) != o.sign(pt[0]) for _, pt in top)
    print("model 2 (sign() without its x0 == 0 branch): noticed by %d of %d random valid points, %d of the %d imaginary_x members with bit 126 "
          "of x1 set (the family has %d)" % (random_hits, len(valid), family_hits, len(top), len(FAM["imaginary_x"])))
    assert len(valid) >= 900 and random_hits == 0 and family_hits == len(top) and 3 * len(top) >= len(FAM["imaginary_x"])


# ---- 4. the mix of outcomes ---------------------------------------------------------------------------------------------------------
def test_outcome_mix_of_the_string_families():
    seeded = [adv.outcome(b) for label, b in FAM["subfield_y"] if label.startswith("seeded")]
    assert len(seeded) == 2 * 150 * 2
    ok = sum(1 for k, _ in seeded if k == "ok")
    off = sum(1 for r in seeded if r == NOT_ON_CURVE)
    print("\nsubfield_y, seeded members: %d ok (%.0f %%), %d not on the curve (%.0f %%), of %d" % (ok, 100.0 * ok / len(seeded), off, 100.0 * off / len(seeded), len(seeded)))
    assert ok + off == len(seeded) and 4 * ok >= len(seeded) and 4 * off >= len(seeded)
    constants = {label: adv.outcome(b) for label, b in FAM["subfield_y"] if label.startswith("constant")}
    assert len(constants) == 10
    for label, got in constants.items():
        if "y = i" in label or "y = -i" in label:
            assert got[0] == "ok", label
        else:
            assert got == ATTRIBUTE_ERROR, label
    assert len([1 for label, _ in FAM["subfield_y"] if label.startswith("v = ")]) == 2 * 2 * len(adv.E_Y) - 12   # v in {0, 1, -1} is one of the constants, listed once
    edge = [adv.outcome(b) for _, b in FAM["edge_words_y"]]
    count = {name: sum(1 for r in edge if (r[0] if r[0] == "ok" else r) == key) for name, key in
             (("ok", "ok"), ("reserved", RESERVED), ("off", NOT_ON_CURVE), ("t == 0", ATTRIBUTE_ERROR))}
    print("edge_words_y: %s of %d" % (count, len(edge)))
    assert all(count.values()) and sum(count.values()) == len(edge)
    assert len([1 for label, _ in FAM["edge_words_y"] if label.startswith("y")]) == 2 * 2 * len(adv.E_Y)
