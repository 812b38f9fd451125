"""Scalars built to reach the states of the device's integer code that random and hand-picked inputs do not (recode.hip.h: mul_shift256 /
decompose, win_reduce / ge256, comb_recode; scalar_n.hip.h: Barrett's quotient).  Pure Python, deterministic; shared by the CPU tests
(test_adversarial_scalars.py, which proves that every family has the property it is for), the fixture generator
(golden/make_adversarial.py) and the GPU tests (test_gpu_adversarial_scalars.py).  Every family returns (label, m) pairs; a label that
starts with "seeded" marks a member drawn from a seeded generator, every other member is constructed."""
import random

import curve4q_oracle as o

N = o.N
ELL = o.ELL
M64 = (1 << 64) - 1
B256 = 1 << 256
QMAX = B256 // N                          # 1568: the largest quotient a 256-bit scalar has
COMB_SHAPES = ((9, 28), (5, 50))          # (w, d) of the fast comb and of the constant-time one (recode.hip.h, CombFast / CombScan)
MU = (1 << 512) // N                      # Barrett's constant (scalar_n.hip.h)
QMAX512 = ((1 << 512) - 1) // N


def words(v, count=4):
    return [(v >> (64 * i)) & M64 for i in range(count)]


def from_words(ws):
    return sum(w << (64 * i) for i, w in enumerate(ws))


def chunk_patterns(D):
    """the D-bit chunk values of comb_ripple: 1, all ones, 0101..., 1010..., 2^(D-1)"""
    alt = sum(1 << i for i in range(0, D, 2))
    return (("1", 1), ("ones", (1 << D) - 1), ("0101", alt), ("1010", (alt << 1) & ((1 << D) - 1)), ("top", 1 << (D - 1)))


def comb_ripple(W, D):
    """Odd k < N whose low D bits are 0...01: every sign digit below D - 1 is -1, so the signed-digit plane of a carry word c is
    -c mod 2^D and the carry of T = low + 2 (T & neg) ripples as far as c's lowest set bit lets it.  k = 1 + 2^(r D) makes plane r
    ripple through all D bits; the chunk patterns vary what the other planes and the carries between them see.  Every k also as
    N - k (even: the comb negates it back) and as k + N, k + 1500 N (through the division by N)."""
    base = [("ripple plane %d" % r, 1 + (1 << (r * D))) for r in range(1, W)]
    pats = chunk_patterns(D)
    for name, p in pats:
        base.append(("chunks %s" % name, (1 + sum(p << (r * D) for r in range(1, W))) % (1 << 245)))
    rng = random.Random(1000 * W + D)
    for t in range(2):                    # two mixtures of the same five patterns, chosen per chunk
        base.append(("chunks mixed %d" % t, (1 + sum(rng.choice(pats)[1] << (r * D) for r in range(1, W))) % (1 << 245)))
    out = []
    for label, k in base:
        assert k % 2 == 1 and k % (1 << (D - 1)) == 1 and 0 < k < N
        for form, m in (("k", k), ("N - k", N - k), ("k + N", k + N), ("k + 1500 N", k + 1500 * N)):
            assert 0 <= m < B256 and m % N
            out.append(("comb %d/%d %s, %s" % (W, D, label, form), m))
    return out


DELTAS = (1, 2, 3, 5, (1 << 63) + 1, (1 << 64) - 1, (1 << 64) + 1, (1 << 127) + 1, (1 << 128) - 1, (1 << 128) + 1, (1 << 191) + 1)
# Seeded j per l_i: 40 in all.  Forty for EACH l_i would be 344 boundary scalars for this family alone and push the families far past the
# 600 or so they are meant to stay within; the constructed members (+-delta, j = 1, 2, 3) are the ones that carry the property.
DECOMPOSE_SEEDED_J = 10


def two_adic(v):
    s = 0
    while v % 2 == 0:
        v, s = v // 2, s + 1
    return s


def decompose_boundary():
    """t_i = (l_i m) >> 256 must be exact.  m = +-delta / l_i makes l_i m = +-delta 2^s (mod 2^256) (2^s the two-adic part of l_i):
    the low half of the product is next to nothing or next to 2^256, where a lost carry or partial product of the low columns flips
    the floor.  ceil(j 2^256 / l_i) and the value before it are where t_i steps from j - 1 to j."""
    out = []
    for i, ell in enumerate(ELL):
        s = two_adic(ell)
        inv = pow(ell >> s, -1, 1 << (256 - s))
        for d in DELTAS:
            for sgn, name in ((1, "+"), (-1, "-")):
                out.append(("decompose l%d %s%#x" % (i + 1, name, d), (sgn * d * inv) % (1 << (256 - s))))
        rng = random.Random(4100 + i)
        js = [("j=%d" % j, j) for j in (1, 2, 3)]
        js += [("seeded j %d" % t, rng.getrandbits(rng.randrange(3, ell.bit_length() - 1)) | 1) for t in range(DECOMPOSE_SEEDED_J)]
        for name, j in js:
            c = -((-j << 256) // ell)
            assert 0 < c < B256
            seeded = "seeded " if name.startswith("seeded") else ""
            out.append(("%sdecompose l%d ceil %s" % (seeded, i + 1, name), c))
            out.append(("%sdecompose l%d ceil %s, minus 1" % (seeded, i + 1, name), c - 1))
    return out


def reduce_equal_words():
    """The restoring division by N 2^k (win_reduce), its comparison (ge256), the +N behind it and the comb's 2N - k: values next to
    N 2^k, values whose words EQUAL those of N 2^k where a borrow arrives (the `b2` term of the borrow), values that agree with
    N 2^k from the top down to one deciding word, every quotient's edge, and remainders whose sum with N has an all-ones word for
    the carry to cross (the `c2` term)."""
    out = []
    for k in range(11):
        s = N << k
        sw = words(s)
        out += [("reduce N 2^%d" % k, s), ("reduce N 2^%d + 1" % k, s + 1), ("reduce N 2^%d - 1" % k, s - 1)]
        for i in (1, 2):                  # word i equal, one less below it (a borrow comes in), one more above it (so the value is >= N 2^k)
            v = list(sw)
            v[i - 1] = (sw[i - 1] - 1) & M64
            v[i + 1] = sw[i + 1] + 1
            assert sw[i - 1] != 0 and v[i + 1] <= M64
            out.append(("reduce N 2^%d equal word %d" % (k, i), from_words(v)))
        for upper in (1, 2, 3):           # the top `upper` words agree; the word below decides, both ways, against what the words under it say
            j = 3 - upper
            assert 0 < sw[j] < M64
            less, more = list(sw), list(sw)
            less[j], less[:j] = sw[j] - 1, [M64] * j
            more[j], more[:j] = sw[j] + 1, [0] * j
            out.append(("reduce N 2^%d upper %d words agree, one less, all ones below" % (k, upper), from_words(less)))
            out.append(("reduce N 2^%d upper %d words agree, one more, zeros below" % (k, upper), from_words(more)))
    for q in (1, 2, 3, 1023, 1024, 1567, 1568):
        for name, r in (("0", 0), ("1", 1), ("2", 2), ("N-2", N - 2), ("N-1", N - 1)):
            if q * N + r < B256:
                out.append(("reduce %d N + %s" % (q, name), q * N + r))
    nw = words(N)
    for i in (1, 2):                      # even r < N: word i of r + N is 2^64 - 1 before the carry out of word i - 1 comes in
        r = [0, 0, 0, 0]
        r[i] = M64 - nw[i]
        r[i - 1] = ((1 << 64) - nw[i - 1] + (1 if i == 1 else 0)) & M64
        v = from_words(r)
        assert v % 2 == 0 and v < N
        out += [("reduce even r, carry crosses word %d" % i, v), ("reduce even r, carry crosses word %d, + 1024 N" % i, v + 1024 * N)]
    assert all(0 <= m < B256 for _, m in out)
    return out


def barrett_boundary():
    """512-bit x = ceil(j 2^512 / mu) and the value before it: where the quotient estimate floor(x mu / 2^512) steps from j - 1 to j"""
    rng = random.Random(4200)
    js = [("j=%d" % j, j) for j in (1, 2, QMAX512, QMAX512 - 1)]
    js += [("seeded j %d" % t, rng.getrandbits(rng.randrange(2, QMAX512.bit_length()))  | 1) for t in range(40)]
    out = []
    for name, j in js:
        c = -((-j << 512) // MU)
        seeded = "seeded " if name.startswith("seeded") else ""
        for tail, x in (("", c), (", minus 1", c - 1)):
            if 0 <= x < (1 << 512):
                out.append(("%sbarrett ceil %s%s" % (seeded, name, tail), x))
    return out


def families256():
    """the three 256-bit families, both comb shapes, in one fixed order"""
    out = []
    for W, D in COMB_SHAPES:
        out += comb_ripple(W, D)
    return out + decompose_boundary() + reduce_equal_words()


def is_seeded(label):
    return label.startswith("seeded")
