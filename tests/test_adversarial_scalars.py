"""The adversarial scalar families of tests/adversarial_scalars.py, before any GPU runs (no GPU needed).

1. Every family has the property it is for.  The models below are plain Python written from the methods' definitions (the comments of
   fourq_amd/csrc/recode.hip.h and scalar_n.hip.h); nothing under fourq_amd/ is imported for them.  They also recompute, and print, how
   far random scalars and the older tests' edge scalars get in the same states, and what three wrong variants of the integer code
   would change (run with -s to see the figures; nothing is asserted on what random scalars do).
2. The two oracles agree on these inputs: oracle/fourq_oracle.c against oracle/curve4q_oracle.py (exact integers) for decompose,
   recode, the fixed-window digits and both MUL_* on G and on a seeded point of order N, with and without a table; Python integers
   for everything modulo N.
3. tests/golden/adversarial.json, the real reference's answers, pins both oracles; where the reference is present the generator must
   reproduce the file byte for byte.
"""
import os
import random

import numpy as np
import pytest

import adversarial_scalars as adv
import curve4q_oracle as o
import oracle_c as oc
import ref_loader
from conftest import GOLDEN, load_golden
from fourq_amd import codec

N = o.N
M64 = (1 << 64) - 1
G1 = o.AffineToR1(o.Gx, o.Gy)
FAM = adv.families256()
MS = [m for _, m in FAM]


# ---- models ---------------------------------------------------------------------------------------------------------------------
def comb_model(m, W, D):
    """mLSB-set comb recoding of m: k = m mod N, replaced by N - k when even (the result is negated).  Plane 0 holds the signs b_i of
    k = sum b_i 2^i (i < D); plane r the signed-digit form T of the running carry word's low D bits, the fixed point of
    T = low + 2 (T & neg) (mod 2^D), reached by iterating from T = low.  Returns (negated, k, planes, rounds each plane needed, last carry)."""
    k = m % N
    negated = k % 2 == 0
    if negated:
        k = N - k
    mask = (1 << D) - 1
    sign = ((k >> 1) & (mask >> 1)) | (1 << (D - 1))
    neg = ~sign & mask
    c = k >> D
    planes, rounds = [sign], []
    for _ in range(1, W):
        low = c & mask
        T, n = low, 0
        while True:
            nxt = (low + ((T & neg) << 1)) & mask
            if nxt == T:
                break
            T, n = nxt, n + 1
        rounds.append(n)
        planes.append(T)
        c = c + ((T & neg) << 1) - T
        assert c % (1 << D) == 0
        c >>= D
    return negated, k, planes, rounds, c


def comb_value(planes, W, D):
    b = [1 if (planes[0] >> i) & 1 else -1 for i in range(D)]
    return sum(b[i] << i for i in range(D)) + sum(((planes[r] >> i) & 1) * b[i] << (r * D + i) for r in range(1, W) for i in range(D))


def t_exact(i, m):
    return ((o.ELL[i] * m) >> 256) & M64


def t_without_columns(i, m, columns):
    """column 4 of the product l_i m when the partial products of the given low columns are left out (their carries with them)"""
    a, w = adv.words(o.ELL[i]), adv.words(m)
    gone = sum(a[x] * w[y] << (64 * (x + y)) for x in range(4) for y in range(4) if x + y in columns)
    return ((o.ELL[i] * m - gone) >> 256) & M64


def divide_by_n(m, borrow_rule="b1 | b2"):
    """Restoring division of a 256-bit m by N 2^k, k = 10 .. 0, word by word; then + N when the remainder is even.  Returns
    (remainder made odd, events): ('borrow', k, i) where word i of the running value equals word i of N 2^k while a borrow comes in
    (the only way the second comparison of the borrow chain fires), ('carry', i) where word i of r + N is 2^64 - 1 before a carry comes in."""
    r = adv.words(m)
    events = []
    for k in range(10, -1, -1):
        s = adv.words(N << k)
        if adv.from_words(r) < adv.from_words(s):
            continue
        borrow = 0
        for i in range(4):
            d1 = (r[i] - s[i]) & M64
            b1 = int(r[i] < s[i])
            d2 = (d1 - borrow) & M64
            b2 = int(d1 < borrow)
            if b2:
                assert r[i] == s[i] and borrow
                events.append(("borrow", k, i))
            r[i] = d2
            borrow = (b1 | b2) if borrow_rule == "b1 | b2" else b1
    if r[0] % 2 == 0:
        n, carry = adv.words(N), 0
        for i in range(4):
            s1 = (r[i] + n[i]) & M64
            c1 = int(s1 < n[i])
            s2 = (s1 + carry) & M64
            c2 = int(s2 < carry)
            if c2:
                assert s1 == M64 and carry
                events.append(("carry", i))
            r[i] = s2
            carry = c1 | c2
    return adv.from_words(r), events


def odd_residue(m):
    r = m % N
    return r if r % 2 else r + N


# ---- 1. the families have the property they are for -------------------------------------------------------------------------------
# the edge scalars tests/test_gpu_comb.py and the double-scalar fixture feed the comb
OLD_EDGES = [0, 1, 2, 3, N - 1, N, N + 1, 2 * N, 2 * N + 1, (1 << 256) - 1, 1 << 255, 1 << 28, (1 << 28) - 1, 1 << 36, (1 << 36) - 1, 1 << 50,
             (1 << 50) - 1, (1 << 252) - 1, 1 << 216, (1 << 245) + 1]


@pytest.mark.parametrize("W,D", adv.COMB_SHAPES)
def test_comb_ripple_reaches_the_last_rounds_of_every_plane(W, D):
    fam = adv.comb_ripple(W, D)
    assert len({m for _, m in fam}) == len(fam) and all(0 < m < (1 << 256) and m % N for _, m in fam)
    for form in ("k", "N - k", "k + N", "k + 1500 N"):
        most = [0] * (W - 1)
        for label, m in fam:
            if not label.endswith(", " + form):
                continue
            negated, k, planes, rounds, c = comb_model(m, W, D)
            assert negated == (form == "N - k") and k % 2 == 1 and 0 < k < N and c == 0, label
            assert comb_value(planes, W, D) == k == (N - m % N if negated else m % N), label
            most = [max(a, b) for a, b in zip(most, rounds)]
        assert all(n >= D - 1 for n in most), (W, D, form, most)
    for label, m in fam:                                           # the named scalar of plane r is the one that does it
        if "ripple plane" in label and label.endswith(", k"):
            r = int(label.split("ripple plane ")[1].split(",")[0])
            assert m == 1 + (1 << (r * D)) and comb_model(m, W, D)[3][r - 1] == D - 1
    # figures, not assertions: what seeded random scalars and the older edge scalars need
    rng = random.Random(5000 + W)
    worst = 0
    for _ in range(100000):
        m = rng.getrandbits(256)
        negated, k, planes, rounds, c = comb_model(m, W, D)
        worst = max(worst, max(rounds))
    edge = max(max(comb_model(m, W, D)[3]) for m in OLD_EDGES)
    print("\ncomb w=%d d=%d: most rounds any plane needs -- family %d, 100000 seeded random scalars %d, older edge scalars %d, of %d"
          % (W, D, D - 1, worst, edge, D))


def test_comb_model_reconstructs_random_scalars():
    rng = random.Random(5100)
    for W, D in adv.COMB_SHAPES:
        for m in [rng.getrandbits(256) for _ in range(300)] + OLD_EDGES + MS:
            negated, k, planes, rounds, c = comb_model(m, W, D)
            assert c == 0 and comb_value(planes, W, D) == k and max(rounds) <= D


def test_decompose_boundary_sits_where_the_floor_flips():
    fam = adv.decompose_boundary()
    deltas = []
    for label, m in fam:
        i = int(label.split(" l")[1][0]) - 1
        ell = o.ELL[i]
        assert 0 <= m < (1 << 256)
        if "ceil" in label:
            lo, hi = (m, m + 1) if label.endswith("minus 1") else (m - 1, m)
            assert (ell * hi >> 256) == (ell * lo >> 256) + 1 and t_exact(i, hi) != t_exact(i, lo), label
        else:
            s = adv.two_adic(ell)
            sgn, d = label.split(" ")[2][0], int(label.split(" ")[2][1:], 16)
            assert (ell * m) % (1 << 256) == ((d if sgn == "+" else -d) << s) % (1 << 256), label
            deltas.append(m)
    assert [adv.two_adic(e) for e in o.ELL] == [0, 0, 2, 6] and len(deltas) == 88
    # what leaving out low partial products would change (figures; the family must notice, random scalars need not)
    rng = random.Random(5200)
    rand = [rng.getrandbits(256) for _ in range(20000)]

    def noticed(ms, columns):
        return sum(any(t_without_columns(i, m, columns) != t_exact(i, m) for i in range(4)) for m in ms)

    all_ms = [m for _, m in fam]
    print("\ndecompose without column 0: noticed by %d of %d random, %d of the 88 +-delta scalars, %d of the family's %d"
          % (noticed(rand, (0,)), len(rand), noticed(deltas, (0,)), noticed(all_ms, (0,)), len(all_ms)))
    print("decompose without columns 0 and 1: noticed by %d of %d random, %d of the 88, %d of the family's %d"
          % (noticed(rand, (0, 1)), len(rand), noticed(deltas, (0, 1)), noticed(all_ms, (0, 1)), len(all_ms)))
    assert noticed(deltas, (0,)) == 29 and noticed(deltas, (0, 1)) == 41       # properties of the constructed members: a weaker family shows here
    assert all(t_without_columns(i, m, ()) == t_exact(i, m) for i in range(4) for m in rand[:200])


def test_reduce_family_has_equal_words_under_a_borrow():
    fam = adv.reduce_equal_words()
    seen_borrow, seen_carry = set(), set()
    for label, m in fam:
        got, events = divide_by_n(m)
        assert got == odd_residue(m), label
        if "equal word" in label:
            k, i = int(label.split("2^")[1].split(" ")[0]), int(label.split("equal word ")[1])
            s, w = adv.words(N << k), adv.words(m)
            assert w[i] == s[i] and w[i - 1] == s[i - 1] - 1 and w[i + 1] == s[i + 1] + 1 and ("borrow", k, i) in events, label
            seen_borrow.add((k, i))
        elif "upper" in label:
            k, upper = int(label.split("2^")[1].split(" ")[0]), int(label.split("upper ")[1][0])
            s, w = adv.words(N << k), adv.words(m)
            assert w[4 - upper:] == s[4 - upper:] and abs(w[3 - upper] - s[3 - upper]) == 1, label
            assert (m < (N << k)) == (w[3 - upper] < s[3 - upper]) == ("one less" in label), label
            if 3 - upper > 0:                                       # the words below say the opposite of the deciding word
                assert (w[0] > s[0]) == (m < (N << k)), label
        elif "carry crosses" in label:
            i = int(label.split("word ")[1][0])
            assert (m % N) % 2 == 0 and ("carry", i) in events, label
            seen_carry.add(i)
        elif " N + " in label:
            q, r = int(label.split(" ")[1]), label.split("+ ")[1]
            assert m // N == q and m % N == {"0": 0, "1": 1, "2": 2, "N-2": N - 2, "N-1": N - 1}[r], label
        else:
            k = int(label.split("2^")[1].split(" ")[0])
            assert m - (N << k) in (-1, 0, 1), label
    assert seen_borrow == {(k, i) for k in range(11) for i in (1, 2)} and seen_carry == {1, 2}
    assert sum(1 for label, _ in fam if "upper" in label) == 66                 # both outcomes of the comparison at every depth, for every k
    # the comb's 2N - k and ge256 see the same shapes through k + N >= N: every even remainder of the family goes that way
    assert sum(1 for _, m in fam if (m % N) % 2 == 0) >= 20
    # a borrow chain that forgets the second comparison (figures for random scalars; the built ones must all notice)
    rng = random.Random(5300)
    rand = [rng.getrandbits(256) for _ in range(20000)]
    built = [m for label, m in fam if "equal word" in label]
    changed = lambda ms: sum(divide_by_n(m, "b1")[0] != odd_residue(m) for m in ms)
    print("\ndivision by N with borrow = b1: changes %d of %d random scalars, %d of the %d built ones" % (changed(rand), len(rand), changed(built), len(built)))
    assert changed(built) == len(built) == 22


def test_barrett_boundary_pairs_flip_the_quotient_estimate():
    fam = dict(adv.barrett_boundary())
    pairs = 0
    for label, x in fam.items():
        assert 0 <= x < (1 << 512)
        if label.endswith(", minus 1"):
            continue
        lo = fam.get(label + ", minus 1")
        assert lo == x - 1 and (x * adv.MU >> 512) == (lo * adv.MU >> 512) + 1, label
        pairs += 1
    assert pairs >= 43 and adv.MU == (1 << 512) // N and adv.MU.bit_length() == 267
    for x in fam.values():                                         # the estimate is Q or Q - 1, as scalar_n.hip.h argues
        assert x // N - (x * adv.MU >> 512) in (0, 1)
    rng = random.Random(5400)
    rand = [rng.getrandbits(512) for _ in range(20000)]
    low = sum(x // N - (x * adv.MU >> 512) for x in rand)
    print("\nBarrett: the estimate is Q - 1 for %d of %d random x (%.1f %%), for %d of the family's %d"
          % (low, len(rand), 100.0 * low / len(rand), sum(x // N - (x * adv.MU >> 512) for x in fam.values()), len(fam)))


def test_family_sizes():
    assert len(FAM) + len(adv.barrett_boundary()) <= 620 and all(0 <= m < (1 << 256) for m in MS)
    assert len({label for label, _ in FAM}) == len(FAM)
    assert FAM == adv.families256()                                 # deterministic


# ---- 2. the oracles agree on these inputs -----------------------------------------------------------------------------------------
def test_c_oracle_recoding_equals_the_python_oracle():
    s = codec.pack_scalars(MS)
    assert [list(map(int, r)) for r in oc.decompose(s)] == [o.decompose(m) for m in MS]
    signs, digits = oc.recode(s)
    wsgn, wind = oc.windowed(s)
    for k, m in enumerate(MS):
        ps, pd = o.recode(o.decompose(m))
        assert list(signs[k]) == ps and list(digits[k]) == pd, hex(m)
        psg, pin = o.recode_windowed(m)
        assert list(wsgn[k]) == psg and list(wind[k]) == pin, hex(m)
        # the digits say what they should: sum d_i 16^i = m mod N made odd
        assert sum((2 * int(i) + 1) * (1 if sg else -1) << (4 * j) for j, (sg, i) in enumerate(zip(psg, pin))) == odd_residue(m)


@pytest.mark.parametrize("base", ["G", "seeded point"])
def test_c_oracle_mul_equals_the_python_oracle(base):
    B = G1 if base == "G" else o.MUL_endo(random.Random(5500).getrandbits(256), G1)
    s = codec.pack_scalars(MS)
    pts = np.repeat(codec.pack_point(B).reshape(1, 20), len(MS), axis=0)
    te, tw = o.table_endo(B), o.table_windowed(B)
    for kind, fn, table in ((oc.ENDO, o.MUL_endo, te), (oc.WINDOWED, o.MUL_windowed, tw)):
        want = [fn(m, B, table=table) for m in MS]                 # the Python oracle's table argument only saves building it again
        assert want[:8] == [fn(m, B) for m in MS[:8]]
        assert codec.unpack_points(oc.mul(kind, s, pts)) == want, (base, kind)
        assert codec.unpack_points(oc.mul(kind, s, None, oc.table(kind, codec.pack_point(B)))) == want, (base, kind, "table")
        assert codec.unpack_table(oc.table(kind, codec.pack_point(B))) == list(table)
        aff = codec.unpack_points(oc.r1_to_affine(codec.pack_points(want, 5)))
        for m, a in zip(MS, aff):                                  # B has order N: both algorithms give [m mod N]B
            assert (a == (o.Ox, o.Oy)) == (m % N == 0)


def test_python_integers_are_the_yardstick_modulo_n():
    """the C oracle's division by N inside MUL_windowed is the only other mod-N code outside the device; its digits were compared above.
    Here: the expectations the GPU tests form for SC_REDUCE512 / SC_MUL / SC_MULSUB are plain `%` on Python integers, and the
    word-by-word long division above agrees with them on every family, the 512-bit one's low halves included."""
    for m in MS + [x & ((1 << 256) - 1) for _, x in adv.barrett_boundary()]:
        assert divide_by_n(m)[0] == odd_residue(m)


# ---- 3. the fixture ---------------------------------------------------------------------------------------------------------------
def fixture_scalars():
    """the order of the fixture's rows: every constructed member, then the seeded ones"""
    return [m for label, m in FAM if not adv.is_seeded(label)] + [m for label, m in FAM if adv.is_seeded(label)]


def fixture_rows():
    rows = load_golden("adversarial.json", raw=True)["rows"]
    out = []
    for m, r in zip(fixture_scalars(), rows):
        pt = lambda h: tuple((int(h[64 * c:64 * c + 32], 16), int(h[64 * c + 32:64 * c + 64], 16)) for c in range(2))
        out.append({"m": m, "decompose": [int(r[0][16 * i:16 * i + 16], 16) for i in range(4)],
                    "signs": [(int(r[1], 16) >> i) & 1 for i in range(65)], "digits": [int(ch) for ch in r[2]],
                    "win_sgn": [int(ch, 16) >> 3 for ch in r[3]], "win_ind": [int(ch, 16) & 7 for ch in r[3]],
                    "endo": pt(r[4]), "windowed": pt(r[5] if len(r) > 5 else r[4])})
    return out


def test_fixture_holds_every_constructed_member_and_fits():
    rows = load_golden("adversarial.json", raw=True)["rows"]
    constructed = sum(1 for label, _ in FAM if not adv.is_seeded(label))
    assert constructed <= len(rows) <= len(FAM) and constructed == 374
    assert os.path.getsize(os.path.join(GOLDEN, "adversarial.json")) <= os.path.getsize(os.path.join(GOLDEN, "mul.json"))


def test_fixture_pins_both_oracles_to_the_reference():
    rows = fixture_rows()
    s = codec.pack_scalars([r["m"] for r in rows])
    dec, (signs, digits), (wsgn, wind) = oc.decompose(s), oc.recode(s), oc.windowed(s)
    te, tw = oc.table(oc.ENDO, codec.pack_point(G1)), oc.table(oc.WINDOWED, codec.pack_point(G1))
    e_aff = codec.unpack_points(oc.r1_to_affine(oc.mul(oc.ENDO, s, None, te)))
    w_aff = codec.unpack_points(oc.r1_to_affine(oc.mul(oc.WINDOWED, s, None, tw)))
    for k, r in enumerate(rows):
        m = r["m"]
        assert o.decompose(m) == r["decompose"] == list(map(int, dec[k])), hex(m)
        assert o.recode(r["decompose"]) == (r["signs"], r["digits"]) and list(signs[k]) == r["signs"] and list(digits[k]) == r["digits"], hex(m)
        assert o.recode_windowed(m) == (r["win_sgn"], r["win_ind"]) and list(wsgn[k]) == r["win_sgn"] and list(wind[k]) == r["win_ind"], hex(m)
        assert e_aff[k] == r["endo"] and w_aff[k] == r["windowed"], hex(m)
    for r in rows[::7]:                                            # the Python oracle's ladders: a seventh of the rows (all of them ran above, against the C oracle)
        assert o.R1toAffine(o.MUL_endo(r["m"], G1)) == r["endo"] and o.R1toAffine(o.MUL_windowed(r["m"], G1)) == r["windowed"]


@pytest.mark.skipif(not ref_loader.available(), reason="the reference is not mounted here")
def test_generator_reproduces_the_fixture_byte_for_byte():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_adversarial", os.path.join(GOLDEN, "make_adversarial.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "adversarial.json")) as fh:
        assert mod.generate() == fh.read()
