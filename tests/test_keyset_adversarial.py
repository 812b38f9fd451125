"""The adversarial keys of tests/keyset_adversarial.py before any GPU runs (no GPU needed).

1. The restatement's statuses (keyset_ref.key_status) reproduce tests/golden/keyset_adversarial.json, made with the real reference's decode,
   DBL and ADD; where the reference is present the generator must reproduce the file byte for byte.
2. Every family is what it is for; the counts are exact.
3. The walk model returns (k + l c) mod N on every row -- what ties it to the kernel's geometry -- and the structured rows reach every
   special case of the complete addition, where 300 random rows reach none."""
import collections
import os
import random

import pytest

import adversarial_points as adv
import curve4q_oracle as o
import keyset_adversarial as ka
import keyset_ref as kref
import ref_loader
import sig_ref
from conftest import GOLDEN, load_golden

N = o.N
REFUSED = kref.KEYSET_NOT_ORDER_N
CODE = {c: sig_ref.BYTES_DECODE_BASE + c for c in (1, 2, 3)}


def statuses():
    return ka.key_statuses([b for _, _, b in ka.all_keys()])


# ---- 1. the fixture -------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_fixture():
    raw = load_golden("keyset_adversarial.json", raw=True)
    keys = ka.all_keys()
    assert raw["keys_sha256"] == ka.keys_sha256()
    assert raw["counts"] == dict(collections.Counter(name for name, _, _ in keys)) and list(raw["counts"]) == ["strings", "shifted", "structured"]
    want = list(bytes.fromhex(raw["statuses"]))
    got = statuses()
    assert len(want) == len(keys)
    assert got == want, [(keys[i][0], keys[i][1], got[i], want[i]) for i in range(len(keys)) if got[i] != want[i]][:8]
    assert os.path.getsize(os.path.join(GOLDEN, "keyset_adversarial.json")) < 8192


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_keyset_adversarial", os.path.join(GOLDEN, "make_keyset_adversarial.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "keyset_adversarial.json")) as fh:
        assert mod.generate() == fh.read()


# ---- 2. the families --------------------------------------------------------------------------------------------------------------------------
def test_strings_statuses_are_exactly_these():
    fam = ka.strings()
    assert len(fam) == 1122 and len({b for _, b in fam}) == 1111
    assert [b for _, b in fam] == [b for _, _, b in adv.all_strings()]                      # duplicates kept, order kept
    st = ka.key_statuses([b for _, b in fam])
    assert collections.Counter(st) == {0: 6, REFUSED: 554, CODE[1]: 24, CODE[2]: 349, CODE[3]: 189}
    assert 24 + 349 + 189 == 562
    accepted = [label for (label, _), s in zip(fam, st) if s == 0]
    zero_half = ["subgroup_zero_half: " + label for label, (x, _) in adv.subgroup_zero_half() if x[1] == 0]
    assert len(zero_half) == 4
    assert sorted(accepted) == sorted(zero_half + ["subfield_y: seeded v 34: y = (0, v), sign bit %d" % s for s in (0, 1)])


def test_the_neutral_point_cannot_be_a_registered_key():
    """The neutral point, the point of order 2 and both points of order 4 have x0 = 0: their encodings do not decode (code 3), as with the
    reference, so [N]O = O never gets as far as being accepted."""
    p = adv.P
    for pt in (adv.NEUTRAL, ((0, 0), (p - 1, 0)), ((0, 1), (0, 0)), ((0, p - 1), (0, 0))):
        assert o.PointOnCurve(pt)
        assert kref.key_status(adv.encode(pt)) == CODE[3], pt
    assert kref.key_status(kref.NEUTRAL_BYTES) == CODE[3]
    by_label = dict(ka.strings())
    for label in ("torsion: order 1", "torsion: order 2", "torsion: order 4: x = i", "torsion: order 4: x = -i"):
        assert kref.key_status(by_label[label]) == CODE[3], label


def test_shifted_keys_decode_and_are_outside_the_subgroup():
    points = ka.shift_points()
    fam = ka.shifted()
    others = [T for _, T in adv.torsion() if T != adv.NEUTRAL]
    assert len(ka.shift_keys()) == 3 and len(points) == len(fam) == 3 * len(others) + 3 == 111
    for (label, _, pt), (_, b) in zip(points, fam):
        assert o.PointOnCurve(pt), label
        assert o.decode(b) == pt, label
    assert ka.key_statuses([b for _, b in fam]) == [REFUSED] * len(fam)
    assert ka.key_statuses(ka.honest_shift_strings()) == [0, 0, 0]
    torsion = dict(adv.torsion())
    orders = {adv.order_in_392(torsion[t]) for _, t, _ in points if t is not None and "full order" not in t}
    assert orders == {2, 4, 7, 14, 28, 56}
    # [N](A + T) = [N]T, a torsion point other than the neutral one: for (-x, -y) = A + (0, -1) the order check lands on (0, -1) itself
    p = adv.P
    _, A = ka.shift_keys()[0]
    assert kref.plain_mul(N, (o.f2_neg(A[0]), o.f2_neg(A[1]))) == ((0, 0), (p - 1, 0))


def test_both_string_families_hold_keys_whose_n_fold_is_the_point_of_order_two():
    """[N]A = (0, -1) has x = 0 like the neutral point: an order check that looked at x alone would accept these keys"""
    p = adv.P
    hits = {}
    for name in ("strings", "shifted"):
        fam = ka.families()[name]
        for (label, b), st in zip(fam, ka.key_statuses([b for _, b in fam])):
            if st == REFUSED and kref.plain_mul(N, o.decode(b)) == ((0, 0), (p - 1, 0)):
                hits.setdefault(name, []).append(label)
    assert hits["strings"] == ["subfield_y: seeded v 111: y = (v, 0), sign bit %d" % s for s in (0, 1)]
    assert sorted(hits["shifted"]) == sorted(["key %d + order 2" % j for j in range(3)] + ["key %d as (-x, -y)" % j for j in range(3)])


def test_structured_keys_are_the_multiples_they_say():
    fam = ka.structured()
    assert len(fam) == len(ka.STRUCTURED_C) == 8
    assert set(ka.STRUCTURED_C) == {1, N - 1, 2, N - 2, (N + 1) // 2, 1 << 7, 1 << 28, (1 << 7) + 1}
    assert (1 << 7) == 1 << ka.E and (1 << 28) == 1 << ka.D                                 # the comb's row and plane strides
    for c, (label, b) in zip(ka.STRUCTURED_C, fam):
        assert b == sig_ref.mul_g_encoded(c), label                                         # the C oracle's encoding = the Python oracle's
    assert ka.key_statuses([b for _, b in fam]) == [0] * 8
    assert fam[0][1] == adv.encode(ka.G) and 2 * ((N + 1) // 2) % N == 1


# ---- 3. the model ----------------------------------------------------------------------------------------------------------------------------
def test_walk_is_the_sum_on_every_row_and_random_rows_reach_no_state():
    for j, k, l, how in ka.structured_rows():
        c = ka.STRUCTURED_C[j]
        assert ka.walk(k, l, c)[0] == (k + l * c) % N, (j, how, hex(k), hex(l))
    rng = random.Random(7711)
    for _ in range(300):
        k, l, c = rng.getrandbits(256), rng.getrandbits(256), rng.randrange(1, N)
        value, counts = ka.walk(k, l, c)
        assert value == (k + l * c) % N
        assert not any(counts.values()), (hex(k), hex(l), hex(c), counts)


def test_structured_rows_reach_every_state():
    rows = ka.structured_rows()
    total = collections.Counter()
    late_doubling = []
    for j, k, l, how in rows:
        trace = []
        _, counts = ka.walk(k, l, ka.STRUCTURED_C[j], trace)
        total.update(counts)
        late_doubling += [(j, how, col, which) for state, col, which in trace if state == "add as doubling" and (col, which) != (6, "A")]
    assert all(total[s] > 0 for s in ka.STATES), total
    assert ka.STRUCTURED_C[1] == N - 1 and ka.STRUCTURED_C[0] == 1
    for k in (1, 5, N + 1, random.Random(7712).getrandbits(256)):
        assert ka.walk(k, k, N - 1)[1] == {"add cancels": 28, "add to neutral": 27, "add as doubling": 0, "dbl of neutral": 6}
        trace = []
        assert ka.walk(k, k, 1, trace)[1] == {"add cancels": 0, "add to neutral": 0, "add as doubling": 1, "dbl of neutral": 0}
        assert trace == [("add as doubling", 6, "A")]                                       # the very first mixed addition
    # a doubling that is NOT the first mixed addition: the last row of the comb, G's entry, under the key [N - 2]G
    assert late_doubling and {(j, col, which) for j, _, col, which in late_doubling} == {(3, 21, "G")}
    assert ka.STRUCTURED_C[3] == N - 2


def test_structured_rows_cover_parities_and_the_neutral_result():
    rows = ka.structured_rows()
    assert 300 <= len(rows) <= 500
    for j, c in enumerate(ka.STRUCTURED_C):
        mine = [(k, l, how) for jj, k, l, how in rows if jj == j]
        assert {ka.parities(k, l) for k, l, _ in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}, j
        assert {how for _, _, how in mine} == {"l = k", "l = N - k", "l = -k / c", "l = 0", "k = 0", "seeded pair"}
        assert any((k + l * c) % N == 0 and k % N for k, l, _ in mine), j                    # the neutral point from two non-zero halves
        assert set(k for k, _, _ in mine) >= set(ka.bucket_ref.EDGE_SCALARS)
        assert any(k >> 255 for k, _, _ in mine)


def test_entry_scalars_are_the_comb_points():
    """column 7 j + i of an odd k: sign, index and 2^i times the entry's scalar add up to k"""
    rng = random.Random(7713)
    for _ in range(20):
        k = rng.getrandbits(256)
        cols = ka.columns(k)
        total = sum(sign * ka.entry_scalar(col // ka.E, u) << (col % ka.E) for col, (sign, u) in enumerate(cols))
        assert total % N == k % N
