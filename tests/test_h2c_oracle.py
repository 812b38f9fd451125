"""Hash to curve on the CPU: the restatement (tests/h2c_ref.py) against the rows the real reference's point functions produced
(tests/golden/h2c.json), the constants against d, the properties of the map, and the header against the binding."""
import os
import random
import re

import curve4q_oracle as o
import h2c_ref as ref

from fourq_amd import constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ref.P
EDGE_U = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (P - 1, P - 1), (1, 2)]


def rows(golden):
    return golden("h2c.json", raw=True)["rows"]


def test_restatement_reproduces_the_golden_rows(golden):
    cases = rows(golden)
    assert 55 <= len(cases) <= 70
    assert {len(c["dst"]) // 2 for c in cases} == {1, 16, 43, 255}
    assert {c["mode"] for c in cases} == {"ro", "nu"}
    for dl in (1, 16, 43, 255):
        lengths = {len(c["msg"]) // 2 for c in cases if len(c["dst"]) // 2 == dl}
        assert lengths >= {0, 1, 15, 16, 17}
        # both sides of the first two growths of b_0's block count: 128 k - (3 + |DST| + 1) - 17 is the last length that fits k blocks
        lasts = [128 * k - dl - 21 for k in range(1, 8) if 128 * k - dl - 21 >= 1][:2]
        for last in lasts:
            assert {last - 1, last, last + 1} <= lengths
            assert {c["mode"] for c in cases if len(c["dst"]) // 2 == dl and len(c["msg"]) // 2 == last + 1} == {"ro", "nu"}
    ints = lambda a: (int(a[0], 16), int(a[1], 16))
    for c in cases:
        dst, msg, mode = bytes.fromhex(c["dst"]), bytes.fromhex(c["msg"]), ref.RO if c["mode"] == "ro" else ref.NU
        u = ref.hash_to_field(msg, dst, mode)
        assert u == [ints(x) for x in c["u"]]
        assert [ref.map_to_curve(x) for x in u] == [(ints(q[0]), ints(q[1])) for q in c["mapped"]]
        assert ref.hash_to_curve_affine(msg, dst, mode) == (ints(c["affine"][0]), ints(c["affine"][1]))
        assert ref.hash_to_curve(msg, dst, mode).hex() == c["point"]


def test_expand_message_xmd_framing():
    # every piece of the framing moves the output; the lengths of the pieces are part of it
    base = ref.expand_message_xmd(b"msg", b"dst", 128)
    assert len(base) == 128 and ref.expand_message_xmd(b"msg", b"dst", 64) != base[:64]          # len_in_bytes is hashed
    assert ref.expand_message_xmd(b"msgd", b"st", 128) != base and ref.expand_message_xmd(b"ms", b"gdst", 128) != base
    for bad in (b"", bytes(256)):
        try:
            ref.expand_message_xmd(b"", bad, 64)
        except ValueError:
            continue
        raise AssertionError("a DST of %d bytes was accepted" % len(bad))
    assert len(ref.expand_message_xmd(b"", bytes(255), 64)) == 64


def test_constants_follow_from_d():
    a = o.f2_neg(ref.ONE)
    amd = o.f2_sub(a, o.d)
    assert o.f2_mul(ref.J, amd) == o.f2_mul((2, 0), o.f2_add(a, o.d))
    assert o.f2_mul(ref.K, amd) == (4, 0)
    assert ref.J == (0x7ffffffffffffc700000000000000509, 0x637a835bf687a14faadcb5733c136818)
    assert ref.K == (0x38ffffffffffffffaf4, 0x1c857ca409785eb055234a8cc3ec97e7)
    # what the device is compiled with (fourq_amd/constants.py -> tools/gen_constants.py -> constants.inc)
    assert constants.d == o.d
    assert (constants.H2C_J, constants.H2C_K, constants.H2C_Z) == (ref.J, ref.K, ref.Z)
    assert constants.H2C_JK == ref.JK and o.f2_mul(constants.H2C_JK, ref.K) == ref.J
    assert constants.H2C_IK2 == ref.IK2 and o.f2_mul(constants.H2C_IK2, o.f2_sqr(ref.K)) == ref.ONE
    assert constants.H2C_SQRT_M5 ** 2 % P == P - ref.norm(ref.Z) == P - 5


def test_z_is_the_first_non_square():
    assert ref.is_square((1, 1)) and not ref.is_square(ref.Z)
    assert ref.is_square((0, 1)) and all(ref.is_square((x, 0)) for x in (0, 1, 2, 3, 5, P - 1))      # GF(p) and i are squares
    # 1 + Z u^2 = 0 has no solution: -1 / Z is not a square
    assert not ref.is_square(o.f2_neg(o.f2_inv(ref.Z)))


def test_sqrt_and_sgn0():
    rng = random.Random(7)
    for a in [(0, 0), (4, 0), (P - 4, 0), (0, 9), (0, P - 9)] + [o.f2_sqr((rng.randrange(P), rng.randrange(P))) for _ in range(40)]:
        assert ref.is_square(a)
        r = ref.sqrt(a)
        assert o.f2_sqr(r) == (a[0] % P, a[1] % P)
        if r != (0, 0):
            assert ref.sgn0(r) != ref.sgn0(o.f2_neg(r))
    assert [ref.sgn0(x) for x in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (2, 1), (P, 1))] == [0, 1, 0, 1, 0, 0, 1]


def test_map_properties():
    rng = random.Random(20261017)
    us = EDGE_U + [(rng.randrange(P), rng.randrange(P)) for _ in range(120)]
    before = dict(ref.REACHED)
    branches = {1: 0, 2: 0}
    for u in us:
        s, t, branch = ref.map_to_montgomery(u)
        branches[branch] += 1
        # on the Montgomery curve, with the sign the branch asks for
        assert o.f2_mul(ref.K, o.f2_sqr(t)) == o.f2_add(o.f2_add(o.f2_mul(o.f2_sqr(s), s), o.f2_mul(ref.J, o.f2_sqr(s))), s)
        assert ref.sgn0(o.f2_mul(t, ref.K_INV)) == (1 if branch == 1 else 0) or t == (0, 0)
        Q = ref.map_to_curve(u)
        assert o.PointOnCurve(o.AffineToR1(*Q))
        assert ref.map_to_curve(o.f2_neg(u)) == Q                                      # even in u
        assert ref.map_to_curve((u[0] + P, u[1] + P)) == Q                             # a function of the residue
    assert min(branches.values()) >= 40
    assert ref.REACHED == before                                                       # no exceptional rule fired on these inputs
    assert ref.map_to_curve((1, 2)) == ((0x63eae08f8a36f8c839f8c8a88255414, 0x188050f38adcdd8c58d393693ff498f8),
                                        (0x6baf5ddc6d5a7d79b22a0aff7c788a8, 0x2beed4aaa95034951838f9089eb0b8e6))
    assert ref.map_to_curve((0, 0)) == ((0x987cc63da76137a68b9280bfc734ae5, 0x5bc8defdfa75c46e7b1278d756af2e97),
                                        (0x6dd18dbbc0626bcd49c1e71f483d33a6, 0x65a62eef0dde7008aa6d3937115b1d4e))


def test_results_have_order_n():
    rng = random.Random(3)
    for i in range(6):
        mode = ref.RO if i % 2 == 0 else ref.NU
        A = ref.hash_to_curve_affine(bytes(rng.getrandbits(8) for _ in range(i * 7)), b"order test", mode)
        assert o.PointOnCurve(o.AffineToR1(*A))
        minus = o.R1toAffine(o.MUL_endo(o.N - 1, o.AffineToR1(*A)))
        assert (ref.canon(minus[0]), ref.canon(minus[1])) == (ref.canon(o.f2_neg(A[0])), A[1])     # [N - 1]P == -P = (-x, y)


def test_the_inputs_with_a_candidate_at_minus_one_over_k():
    """x = -1/K is s = -1, where the rational map's y = (s - 1) / (s + 1) has no denominator.  Both inputs exist; in both the OTHER candidate
    is the one selected (g(-1/K) is not a square), so the (0, 1) rule is not reached through them."""
    special = ref.special_inputs()
    assert [which for _, which in special] == [1, 2]
    minus_ik = o.f2_neg(ref.K_INV)
    assert not ref.is_square(ref.g_of(minus_ik))
    before = dict(ref.REACHED)
    for u, which in special:
        x1, x2 = ref.elligator2_candidates(u)
        assert (x1, x2)[which - 1] == ref.canon(minus_ik)
        s, t, branch = ref.map_to_montgomery(u)
        assert branch == 3 - which and ref.canon(o.f2_add(s, ref.ONE)) != (0, 0)
        assert o.PointOnCurve(o.AffineToR1(*ref.map_to_curve(u)))
    assert ref.REACHED == before
    # the rule itself, where it does apply: t = 0 (the point (0, 0) of the Montgomery curve, of order 2) and s = -1
    assert ref.montgomery_to_edwards((0, 0), (0, 0)) == ((0, 0), (1, 0))
    assert ref.montgomery_to_edwards((P - 1, 0), (5, 7)) == ((0, 0), (1, 0))
    assert ref.REACHED["neutral"] == before["neutral"] + 2


def test_the_self_test_vector_is_the_restatements():
    from fourq_amd import h2c
    assert ref.hash_to_curve(h2c.KAT_MSG, h2c.KAT_DST, ref.RO).hex() == h2c.KAT_POINT


def test_header_and_binding_declare_the_same_new_symbols():
    from fourq_amd import _lib
    header = open(os.path.join(ROOT, "include", "fourq_amd.h")).read()
    declared = set(re.findall(r"\b(fourq_\w+)\s*\(", header))
    new = {"fourq_hash_to_field_batch", "fourq_map_to_curve_batch", "fourq_hash_to_curve_batch", "fourq_hash_to_curve_affine_batch"}
    new |= {n + "_dev" for n in new}
    assert new <= declared and new <= set(_lib.PROTOTYPES)
    assert {n for n in declared if "hash_to" in n or "map_to" in n} == new == {n for n in _lib.PROTOTYPES if "hash_to" in n or "map_to" in n}
    for name in ("FOURQ_H2C_RO 0", "FOURQ_H2C_NU 1", "FOURQ_H2C_MAX_DST 255"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", header), name
    assert (_lib.H2C_RO, _lib.H2C_NU, _lib.H2C_MAX_DST) == (0, 1, 255)
    assert re.search(r"FOURQ_PT_MAP_ELL2\s*=\s*47\b", header) and _lib.PRIM["PT_MAP_ELL2"] == 47
    # the message arguments are those of fourq_sha512_batch, behind (ctx, dst, dst_len, mode)
    sha = _lib.PROTOTYPES["fourq_sha512_batch"][1]
    for n in new - {"fourq_map_to_curve_batch", "fourq_map_to_curve_batch_dev"}:
        args = _lib.PROTOTYPES[n][1]
        assert args[4:] == sha[1:] and len(args) == 10, n
    assert "#define FOURQ_ABI_VERSION 600" in header and _lib.ABI_VERSION == 600
