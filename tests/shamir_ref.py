"""Threshold sharing as include/fourq_amd.h writes it out ("threshold sharing"), restated on Python integers and the oracle modules:
Horner's rule, the Lagrange coefficients with pow(d, -1, N), both combines, the Feldman commitments and their check; the point sums are
oracle/curve4q_oracle.py's MUL_endo, ADD, encode and decode, as in the other *_ref.py files, and decode's statuses tests/sig_ref.py's.
A helper for the threshold tests, not the code under test.

Every function that stands for a library call returns what the library reports, statuses included.  Arrays that hold one item per
(party, row) are lists of party blocks: item (i, r) is [i][r].
"""
import curve4q_oracle as o
import sig_ref

N = o.N
MAX_T, ID_ZERO, ID_REPEATED = 4096, 144, 160
DECODE_BASE, SIG_S_RANGE = 16, 32
GEN = (o.Gx, o.Gy)
ZERO32 = bytes(32)
NEUTRAL32 = bytes([1] + [0] * 31)
REFUSED_NEUTRAL = DECODE_BASE + sig_ref.DECODE_REF_ATTRIBUTE_ERROR        # what a grouped sum says of the neutral point's encoding


def enc(P):
    return bytes(o.encode(P[0], P[1]))


def horner(coeffs, x):
    """sum_j coeffs[j] x^j mod N, from the top coefficient down"""
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % N
    return acc


def shares(polys, ids):
    """(blocks, status): blocks[p][r] = polys[r] at ids[p]; an id 0 gives ID_ZERO and a block of zeros"""
    blocks = [[0 if x == 0 else horner(poly, x) for poly in polys] for x in ids]
    return blocks, [ID_ZERO if x == 0 else 0 for x in ids]


def set_status(ids):
    return ID_ZERO if 0 in ids else ID_REPEATED if len(set(ids)) != len(ids) else 0


def lagrange(ids):
    """(lambda, status) of one set: lambda_i = prod_(j != i) x_j / (x_j - x_i) mod N; all zero under a status"""
    st = set_status(ids)
    if st:
        return [0] * len(ids), st
    out = []
    for i, xi in enumerate(ids):
        num = den = 1
        for j, xj in enumerate(ids):
            if j != i:
                num, den = num * xj % N, den * (xj - xi) % N
        out.append(num * pow(den, -1, N) % N)
    return out, 0


def combine(ids, blocks):
    """(out, status): out[r] = sum_i lambda_i blocks[i][r] mod N"""
    lam, st = lagrange(ids)
    return [sum(l * blocks[i][r] for i, l in enumerate(lam)) % N for r in range(len(blocks[0]))], st


def point_sum(scalars, points32):
    """(encode(sum [k]decode(P)), status) as fourq_msm_bytes_batch defines them for one group: 16 + the largest decode code and a zero row;
    the complete addition, the neutral point an ordinary result"""
    worst, acc = 0, None
    for k, b in zip(scalars, points32):
        st, P = sig_ref.decode_status(bytearray(b))
        worst = max(worst, st)
        if st == 0:
            T = o.MUL_endo(k, o.AffineToR1(P[0], P[1]))
            acc = T if acc is None else o.ADD(acc, o.R1toR2(T))
    return (ZERO32, worst) if worst else (enc(o.R1toAffine(acc)), 0)


def combine_points(ids, blocks32):
    """(out32, status) per row: out32[r] = encode(sum_i [lambda_i]decode(blocks32[i][r])); a bad id set marks and zeroes every row"""
    lam, st = lagrange(ids)
    n = len(blocks32[0])
    if st:
        return [ZERO32] * n, [st] * n
    rows = [point_sum(lam, [block[r] for block in blocks32]) for r in range(n)]
    return [r[0] for r in rows], [r[1] for r in rows]


def commitments(poly):
    """encode([a_j]G) per coefficient"""
    return [enc(o.R1toAffine(o.MUL_endo(a, o.AffineToR1(*GEN)))) for a in poly]


def public_share(commits32, x):
    """(out32, status): encode(sum_j [x^j mod N]decode(C_j)); ID_ZERO first"""
    if x == 0:
        return ZERO32, ID_ZERO
    return point_sum([pow(x, j, N) for j in range(len(commits32))], commits32)


def verify(commits32, x, share):
    """(ok, status): public_share's status, else SIG_S_RANGE for a share not below N"""
    pub, st = public_share(commits32, x)
    if st == 0 and share >= N:
        st = SIG_S_RANGE
    if st:
        return 0, st
    return int(pub == enc(o.R1toAffine(o.MUL_endo(share, o.AffineToR1(*GEN))))), 0


def horner_step_words(acc, x, a, mu):
    """One step of shamir.hip.h's sc_horner_step on integers, as the kernel computes it: the quotient from the top words of v and of mu,
    two conditional subtractions.  Returns (result, quotient estimate, v)"""
    v = acc * x + a
    q = ((v >> 192) * (mu >> 192)) >> 128
    r = (v - q * N) % (1 << 256)
    for _ in range(2):
        r = r - N if r >= N else r
    return r, q, v
