"""The bucket route of the grouped sums (fourq_bucketsum_*, fourq_amd/csrc/bucket.hip.h) restated on the Python oracle, step by step, and
the scalar pool that tests/test_gpu_bucket_sum.py runs on the device.  No GPU, nothing from the library under test.

    1  v = decompose(k): four sub-scalars below 2^64
    2+3  per (sub-scalar j, window w): bucket[d] = sum of the points whose digit is d, digit 0 skipped
    4  sum_d d bucket[d] per column, 16 consecutive buckets d0 + 1 .. d0 + 16 at a time, highest first: run += bucket, tot += run,
       the chunk's share tot + [d0]run with [d0] by double-and-add over the window's c bits
    5  S_j by Horner over the windows, top first, c doublings between them; S_0 + phi(S_1) + psi(S_2) + psi(phi(S_3))

Points travel as the oracle's R1 tuples.  An addition with the neutral TUPLE OBJECT below returns the other operand: an exact shortcut (the
neutral is the neutral), which keeps the empty buckets of a 12-bit window from costing a field multiplication each."""
import curve4q_oracle as o

NEUTRAL = ((0, 0), (1, 0), (1, 0), (0, 0), (1, 0))
TOP = (1 << 256) - 1
EDGE_SCALARS = (0, 1, o.N, TOP, o.N - 1, o.N + 1)
CHUNK = 16


def add(P, Q):
    if P is NEUTRAL:
        return Q
    if Q is NEUTRAL:
        return P
    return o.ADD(P, o.R1toR2(Q))


def digit(v, w, c):
    return (v >> (w * c)) & ((1 << c) - 1)


def sub_scalars(k):
    v = o.decompose(k)
    assert len(v) == 4 and all(0 <= x < 1 << 64 for x in v), (k, v)
    return v


def column_sum(buckets, c):
    """sum_d d buckets[d] for d = 1 .. 2^c - 1 by chunks of 16 buckets; buckets: {digit: R1 point}"""
    B = 1 << c
    col = NEUTRAL
    for d0 in range(0, B, CHUNK):
        run = tot = NEUTRAL
        for i in range(CHUNK, 0, -1):
            run = add(run, buckets.get(d0 + i, NEUTRAL) if d0 + i < B else NEUTRAL)
            tot = add(tot, run)
        acc = NEUTRAL
        if run is not NEUTRAL:
            for b in range(c - 1, -1, -1):
                acc = acc if acc is NEUTRAL else o.DBL(acc)
                if (d0 >> b) & 1:
                    acc = add(acc, run)
        col = add(col, add(tot, acc))
    return col


def bucket_sum(ks, points, c, endo=(o.phi, o.psi)):
    """canonical affine sum_i MUL_endo(k_i, P_i) over affine points, by steps 1-5 with window c"""
    W = -(-64 // c)
    vs = [sub_scalars(k) for k in ks]
    lifted = [o.AffineToR1(*P) for P in points]
    S = []
    for j in range(4):
        cols = []
        for w in range(W):
            buckets = {}
            for v, P in zip(vs, lifted):
                d = digit(v[j], w, c)
                if d:
                    buckets[d] = add(buckets.get(d, NEUTRAL), P)
            cols.append(column_sum(buckets, c))
        s = cols[W - 1]
        for w in range(W - 2, -1, -1):
            for _ in range(c):
                s = s if s is NEUTRAL else o.DBL(s)
            s = add(s, cols[w])
        S.append(s)
    phi, psi = endo
    ends = [S[0]] + [NEUTRAL if s is NEUTRAL else f(s) for s, f in ((S[1], phi), (S[2], psi), (S[3], lambda p: psi(phi(p))))]
    total = NEUTRAL
    for e in ends:
        total = add(total, e)
    return o.R1toAffine(total)


def ladder_sum(ks, points):
    """R1toAffine(sum_i MUL_endo(k_i, AffineToR1(P_i))): what fourq_msm_* computes"""
    total = NEUTRAL
    for k, P in zip(ks, points):
        total = add(total, o.MUL_endo(k, o.AffineToR1(*P)))
    return o.R1toAffine(total)


def times(k, P):
    """plain [k]P by double-and-add, P an R1 tuple"""
    acc = NEUTRAL
    for b in range(k.bit_length() - 1, -1, -1):
        acc = acc if acc is NEUTRAL else o.DBL(acc)
        if (k >> b) & 1:
            acc = add(acc, P)
    return acc


def is_neutral(P):
    x, y = o.R1toAffine(P)
    return x == (0, 0) and y == (1, 0)


def outside_subgroup_points(seed, count):
    """`count` (32-byte string, affine point) pairs: seeded random strings that the oracle's decode accepts and whose point has [N]P != O"""
    import random
    rng, out = random.Random(seed), []
    while len(out) < count:
        enc = bytes(rng.getrandbits(8) for _ in range(32))
        try:
            P = o.decode(enc)
        except Exception:
            continue
        if not is_neutral(times(o.N, o.AffineToR1(*P))):
            out.append((enc, P))
    return out


def plant_edges(k):
    """the six edge scalars at fixed places of a scalar list, front and back, as tests/test_gpu_msm.py plants them"""
    for i, e in enumerate(EDGE_SCALARS):
        k[1 + 7 * i] = e
        k[len(k) - 1 - 5 * i] = e
    return k


def pool_scalars(count, seed=7400):
    from bench import seeded_scalars
    from fourq_amd import codec
    return plant_edges(codec.unpack_scalars(seeded_scalars(seed, count)))
