"""The closed-form recoders of fourq_amd/csrc/recode.hip.h on the CPU.  recode() and recode_nibbles() are plain C++ behind one qualifier
macro, so tests/c/recode_check.cpp includes the shipped header, compiles for the host and holds both against the bit-serial loop they
replaced (curve4q.py:358-380), which lives on inside that program.  Inputs: v = decompose(m) of every family of adversarial_scalars.py,
the grid of edge words below, and a million seeded rows.  The results of the file rows come back and are held against the Python oracle
as well, so the program's own loop is pinned too.  The same program once more under AddressSanitizer + UndefinedBehaviorSanitizer: it is
stand-alone, nothing is preloaded."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import adversarial_scalars as adv
import curve4q_oracle as o
from conftest import ROOT

M64 = (1 << 64) - 1
A5 = 0x5555555555555555
VJ = (0, 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64, A5, A5 << 1)
V0 = (1, 3, M64, A5, (A5 << 1) | 1)                 # 0xAA...AB: decompose() hands over an odd first word
N_RANDOM = 1 << 20


def grid_rows():
    return [[v0, v1, v2, v3] for v0 in V0 for v1, v2, v3 in itertools.product(VJ, repeat=3)]


def nibble_words(signs, digits):
    """what recode_nibbles must return for the oracle's 65 signs and digits: step i is nibble i % 8 of word i / 8, bit 3 set when the
    step subtracts"""
    return [sum((digits[8 * k + j] | ((1 - signs[8 * k + j]) << 3)) << (4 * j) for j in range(8)) for k in range(8)]


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "fourq_amd", "csrc")] + extra +
                   [os.path.join(ROOT, "tests", "c", "recode_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recode_check")
    r = [o.decompose(m) for _, m in adv.families256()] + grid_rows()
    path = tmp / "rows.bin"
    np.array(r, dtype=np.uint64).tofile(path)
    return tmp, str(path), r


def _run(exe, path, out):
    proc = subprocess.run([exe, path, out, str(N_RANDOM)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert "runtime error" not in proc.stderr and "Sanitizer" not in proc.stderr, proc.stderr[-4000:]
    seen = {}
    for line in proc.stdout.splitlines():
        f = line.split()
        seen[tuple(f[:-1]) if f[0] in ("file", "random") else f[0]] = int(f[-1]) if f[0] != "rows" else (int(f[1]), int(f[2]))
    return seen


def _conditions(seen, n_rows):
    assert seen["rows"] == (n_rows, N_RANDOM) and N_RANDOM >= 10 ** 6 and seen["differ"] == 0
    for what in ("file", "random"):
        for top in range(8):
            assert seen[(what, "top", str(top))] > 0, (what, top)
        for j in (1, 2, 3):
            for c in (0, 1):
                assert seen[(what, "carry", str(j), str(c))] > 0, (what, j, c)


def test_shipped_recoders_equal_the_bit_serial_loop_and_the_oracle(rows):
    tmp, path, r = rows
    out = str(tmp / "out.bin")
    seen = _run(_build(tmp, "recode_check", []), path, out)
    _conditions(seen, len(r))
    got = np.fromfile(out, dtype=np.uint64).reshape(len(r), 14)
    tops = set()
    for v, g in zip(r, got):
        signs, digits = o.recode(v)
        sign, d0, d1, d2, top = (int(x) for x in g[:5])
        assert [(sign >> i) & 1 for i in range(64)] == signs[:64] and signs[64] == 1, v
        assert [((d0 >> i) & 1) | (((d1 >> i) & 1) << 1) | (((d2 >> i) & 1) << 2) for i in range(64)] + [top] == digits, v
        assert [int(x) for x in g[5:13]] == nibble_words(signs, digits) and int(g[13]) == digits[64], v
        tops.add(digits[64])
    assert tops == set(range(8))


def test_shipped_recoders_under_the_sanitizers(rows):
    tmp, path, r = rows
    exe = _build(tmp, "recode_check_san", ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"])
    _conditions(_run(exe, path, str(tmp / "out_san.bin")), len(r))


def test_top_digits_0_and_2_never_come_out_of_decompose():
    """Why the GPU test of the ladders (test_gpu_recode_closed_form.py) asks for six top digits and not eight.  The top digit is
    c1 + 2 c2 + 4 c3, c_j the carry out of v_j + ~(v_0 >> 1): c_j = 0 needs v_j <= v_0 / 2.  decompose(m) is offset + sum_j f_j b_j with
    b_j the rows of BASIS as signed words, offset one of OFFSET_C / OFFSET_CP and f_j = frac(l_j m / 2^256) (up to 2^-190: the l_j are
    rounded), a point of a parallelepiped.  Over the whole box f in [0, 1]^4 -- exactly, in rational arithmetic, at the vertices of the
    polytope the second inequality cuts from the box -- 2 v_3 <= v_0 together with 2 v_1 <= v_0 has no solution: the smaller 2 v_1 - v_0 gets
    there is above 2^62, so neither rounding nor the parity of v_0 >> 1 is near enough to matter.  Digits 0 and 2 need c1 = c3 = 0."""
    from fractions import Fraction

    def signed(x):
        x %= 1 << 64
        return x - (1 << 64) if x >> 63 else x
    B = [[signed(x) for x in row] for row in o.BASIS]
    for offset in (o.OFFSET_C, o.OFFSET_CP):
        off = [x % (1 << 64) for x in offset]
        # 2 v_a - v_0 as (constant, coefficients of f)
        g1, g3 = ((2 * off[a] - off[0], [2 * B[j][a] - B[j][0] for j in range(4)]) for a in (1, 3))
        value = lambda g, f: g[0] + sum(c * x for c, x in zip(g[1], f))
        vertices = [tuple(map(Fraction, f)) for f in itertools.product((0, 1), repeat=4) if value(g3, f) <= 0]
        for k in range(4):                    # ... and where g3 = 0 crosses an edge of the box
            for rest in itertools.product((0, 1), repeat=3):
                f = list(rest[:k]) + [0] + list(rest[k:])
                if g3[1][k]:
                    t = Fraction(-value(g3, f), g3[1][k])
                    if 0 <= t <= 1:
                        f[k] = t
                        vertices.append(tuple(map(Fraction, f)))
        assert all(value(g1, f) > 1 << 62 for f in vertices), offset      # an empty list: c3 = 0 alone is out of reach with this offset
    # the grid of the tests above does reach them: recode() takes any four words
    assert {o.recode(r)[1][64] for r in grid_rows()} == set(range(8))
