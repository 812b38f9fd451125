"""Arithmetic modulo the group order on the device (scalar_n.hip.h) through the primitive ABI, against Python integers."""
import random

import numpy as np
import pytest

import curve4q_oracle as o

pytestmark = pytest.mark.gpu

N = o.N
M64 = (1 << 64) - 1


def words(v, count):
    return [(v >> (64 * i)) & M64 for i in range(count)]


def value(row):
    return sum(int(w) << (64 * i) for i, w in enumerate(row))


def edge_values(bits):
    top = (1 << bits) - 1
    vals = [0, 1, 2, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, top, top - 1, (1 << 256) - 1, 1 << 255, (1 << 246) - 1, 1 << 246]
    q = top // N
    for k in (q, q - 1, q // 2, 3, 1 << 10, (1 << 266) - 1 if bits > 256 else 7):
        if k * N + 1 <= top:
            vals += [k * N - 1, k * N, k * N + 1]
    for i in range(bits // 64):                      # single-bit and all-ones words in every position
        vals += [1 << (64 * i), 1 << (64 * i + 63), M64 << (64 * i), top ^ (M64 << (64 * i))]
    return [v for v in vals if 0 <= v <= top]


def run(eng, op, rows, in_words):
    x = np.array([sum((words(v, w) for v, w in zip(r, in_words)), []) for r in rows], dtype=np.uint64)
    return [value(r) for r in eng.prim(op, x)]


def test_reduce512(eng):
    rng = random.Random(67)
    vals = edge_values(512) + [rng.getrandbits(512) for _ in range(4000)] + [rng.getrandbits(rng.randrange(1, 513)) for _ in range(1000)]
    got = run(eng, "SC_REDUCE512", [(v,) for v in vals], (8,))
    bad = [i for i, (g, v) in enumerate(zip(got, vals)) if g != v % N]
    assert not bad, [hex(vals[i]) for i in bad[:4]]


def test_mul(eng):
    rng = random.Random(69)
    e = edge_values(256)
    rows = [(a, b) for a in e[:24] for b in e[:24]] + [(rng.choice(e), rng.getrandbits(256)) for _ in range(500)]
    rows += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(4000)]
    got = run(eng, "SC_MUL", rows, (4, 4))
    bad = [i for i, (g, (a, b)) in enumerate(zip(got, rows)) if g != a * b % N]
    assert not bad, [tuple(map(hex, rows[i])) for i in bad[:4]]


def test_mulsub(eng):
    rng = random.Random(68)
    e = edge_values(256)
    rows = [(r, a, h) for r in e[:14] for a in e[:14] for h in (0, 1, N - 1, N, (1 << 256) - 1)]
    rows += [(rng.choice(e), rng.choice(e), rng.choice(e)) for _ in range(1000)]
    rows += [(rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256)) for _ in range(4000)]
    rows += [(a * h % N, a, h) for a, h in ((rng.getrandbits(256), rng.getrandbits(256)) for _ in range(50))]      # r = a h: the result is 0
    got = run(eng, "SC_MULSUB", rows, (4, 4, 4))
    bad = [i for i, (g, (r, a, h)) in enumerate(zip(got, rows)) if g != (r - a * h) % N]
    assert not bad, [tuple(map(hex, rows[i])) for i in bad[:4]]
    assert all(g < N for g in got)
