"""Pins what the GPU tests of the double-scalar multiplication expect, before any GPU runs (no GPU needed).

tests/golden/double_mul.json holds the real reference's R1toAffine(ADD(MUL_endo(k, G), R1toR2(MUL_endo(l, P)))) for about 64 cases
(tests/golden/make_double_mul.py).  The Python oracle must reproduce it, and where P = [t]G the same point must come out of the
group law [k]G + [l][t]G = [(k + l t) mod N]G -- the identity tests/test_gpu_double_mul.py builds its large batches on.
"""
import random

import numpy as np

import curve4q_oracle as o
import oracle_c as oc
from fourq_amd import codec

G1 = o.AffineToR1(o.Gx, o.Gy)
NEUTRAL_ENC = bytes([1] + [0] * 31)


def double_mul(k, l, P):
    return o.R1toAffine(o.ADD(o.MUL_endo(k, G1), o.R1toR2(o.MUL_endo(l, o.AffineToR1(*P)))))


def test_fixture_covers_the_cases_it_promises(golden):
    cases = golden("double_mul.json")["cases"]
    labels = {c["_label"] for c in cases}
    assert len(cases) >= 60
    for want in ("random", "k edge", "l edge", "k = l = 0 (neutral result)", "doubling", "sum neutral", "P = G", "P neutral", "P outside the order-N subgroup"):
        assert want in labels
    edges = {0, 1, o.N - 1, o.N, o.N + 1, (1 << 256) - 1}
    assert edges <= {c["k"] for c in cases} and edges <= {c["l"] for c in cases}
    outside = {c["P"] for c in cases if c["_label"].startswith("P outside")}
    assert len(outside) == 2 and all(o.PointOnCurve(P) for P in outside)
    # outside the subgroup indeed: [N]P is not the neutral point
    assert all(o.R1toAffine(o.MUL_windowed(o.N - 1, o.AffineToR1(*P))) != (o.f2_neg(P[0]), P[1]) for P in outside)


def test_oracle_reproduces_the_reference(golden):
    for c in golden("double_mul.json")["cases"]:
        R = double_mul(c["k"], c["l"], c["P"])
        assert R == c["R"], c["_label"]
        assert bytes(o.encode(*c["P"])).hex() == "%064x" % c["P_enc"] and bytes(o.encode(*R)).hex() == "%064x" % c["R_enc"], c["_label"]
        if c["_label"].startswith(("sum neutral", "k = l = 0")):
            assert R == ((0, 0), (1, 0)) and bytes(o.encode(*R)) == NEUTRAL_ENC


def test_decode_verdicts_of_the_fixture_match_the_oracle(golden):
    for c in golden("double_mul.json")["cases"]:
        enc = bytes.fromhex("%064x" % c["P_enc"])
        try:
            ok = o.decode(enc) == c["P"]
        except Exception as exc:
            assert c["_P_decode"].startswith(type(exc).__name__), c["_label"]
        else:
            assert ok and c["_P_decode"] == "ok", c["_label"]


def test_group_law_gives_the_same_point():
    """[k]G + [l][t]G == [(k + l t) mod N]G through both oracles, including doubling ([k]G == [l]P), inverse points and a neutral half."""
    rng = random.Random(77)
    rows = [(rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256)) for _ in range(12)]
    l, t = rng.getrandbits(256), rng.getrandbits(200)
    rows += [((l * t) % o.N, l, t), ((-l * t) % o.N, l, t), (0, l, t), (rng.getrandbits(256), 0, t), (0, 0, t), (5, 7, 0), (o.N, o.N + 1, t)]
    g1 = codec.pack_points([G1], 5)
    for k, l, t in rows:
        P = o.R1toAffine(o.MUL_endo(t, G1))
        want = o.R1toAffine(o.MUL_endo((k + l * t) % o.N, G1))
        assert double_mul(k, l, P) == want
        c_want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars([(k + l * t) % o.N]), g1))
        assert codec.unpack_points(c_want) == [want]
    assert double_mul((l * t) % o.N, l, o.R1toAffine(o.MUL_endo(t, G1))) == o.R1toAffine(o.DBL(o.MUL_endo((l * t) % o.N, G1)))
    assert double_mul((-l * t) % o.N, l, o.R1toAffine(o.MUL_endo(t, G1))) == ((0, 0), (1, 0))


def test_c_oracle_encode_matches_the_python_oracle(golden):
    cases = golden("double_mul.json")["cases"]
    rows = codec.pack_points([c["R"] for c in cases], 2)
    assert [bytes(r).hex() for r in oc.encode(rows)] == ["%064x" % c["R_enc"] for c in cases]
    assert np.array_equal(oc.encode(codec.pack_points([((0, 0), (1, 0))], 2))[0], np.frombuffer(NEUTRAL_ENC, dtype=np.uint8))
