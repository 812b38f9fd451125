"""The closed-form recoders (fourq_amd/csrc/recode.hip.h) on the device.  tests/test_recode_host.py holds the same code, compiled for the
host, against the bit-serial loop on a million rows; here the compiled gfx950 code is asked directly -- the primitives SC_RECODE (the
planes: the constant-time and pair-lane ladders) and SC_RECODE_NIBBLES (the nibble stream of the fused ladders) on a grid of edge words
against the Python oracle's signs and digits -- and then through the one-lane fused kernels, whose ladders read those digits: MUL_endo, DH
and a mixed batch of 640 elements against the C oracle.  Their scalars are picked from a seeded pool so that every value the top digit CAN take
in a multiplication occurs at least 40 times: that is 1, 3, 4, 5, 6 and 7.  The top digit is c1 + 2 c2 + 4 c3 with c_j the carry out of
v_j + ~(v_0 >> 1), and decompose() never returns a v with c1 = c3 = 0 (test_recode_host.py proves it from the lattice basis; two million
seeded scalars give 0 and 2 not once, 4 in 0.24 % of them), so the digits 0 and 2 are reached by the primitives only, on the grid.  Both
selection modes (the `eng` fixture)."""
import itertools

import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_scalars
from fourq_amd import codec

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
A5 = 0x5555555555555555
VJ = (0, 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64, A5, A5 << 1)
V0 = (1, 3, M64, A5, (A5 << 1) | 1)
N = 640
REACHABLE_TOPS = (1, 3, 4, 5, 6, 7)
G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
HOOKS = ("FOURQ_PAIR_MAX", "FOURQ_QUAD_MAX", "FOURQ_MIXED_QUEUE")

_cache = {}


def shared():
    """inputs and expectations, computed once for both selection modes"""
    if _cache:
        return _cache
    c = _cache
    # every (v1, v2, v3) of the edge words; the first word walks through its five values with them, and every first word meets the 64
    # combinations of the two extremes' neighbours again: 512 + 5 * 64 + 5 * 8 rows
    triples = list(itertools.product(VJ, repeat=3))
    rows = [[V0[k % 5]] + list(t) for k, t in enumerate(triples)]
    rows += [[v0] + list(t) for v0 in V0 for t in itertools.product((0, 1, M64 - 1, M64), repeat=3)]
    rows += [[v0, a, a, a] for v0 in V0 for a in VJ]
    c["v"] = np.array(rows, dtype=np.uint64)
    c["want"] = [o.recode(r) for r in rows]
    assert {d[64] for _, d in c["want"]} == set(range(8))
    pool = seeded_scalars(9101, 1 << 15)
    top = np.asarray(oc.recode(pool)[1])[:, 64]
    pick = np.concatenate([np.flatnonzero(top == t)[:40] for t in REACHABLE_TOPS])
    pick = np.concatenate([pick, np.setdiff1d(np.arange(len(pool)), pick)[:N - len(pick)]])
    c["S"] = pool[np.sort(pick)]
    tops = [o.recode(o.decompose(m))[1][64] for m in codec.unpack_scalars(c["S"])]
    assert len(c["S"]) == N and all(tops.count(t) >= 40 for t in REACHABLE_TOPS) and set(tops) == set(REACHABLE_TOPS), sorted(set(tops))
    te = oc.table(oc.ENDO, G1_WORDS)
    c["table"] = te
    c["pts"] = oc.mul(oc.ENDO, seeded_scalars(9102, N), None, te)           # projective points of order N
    c["aff"] = oc.r1_to_affine(c["pts"])
    c["mul"] = oc.mul(oc.ENDO, c["S"], c["pts"])
    c["dh"] = oc.dh(oc.ENDO, c["S"], c["aff"])
    c["flags"] = (np.arange(N) % 3 != 0).astype(np.uint8)
    c["mixed"] = np.where(c["flags"][:, None] == 0, oc.mul(oc.ENDO, c["S"], None, te), c["mul"])
    return c


def test_both_recoding_primitives_on_the_edge_grid(eng):
    c = shared()
    assert 800 <= len(c["v"]) <= 1200
    planes = eng.prim("SC_RECODE", c["v"])
    nibbles = eng.prim("SC_RECODE_NIBBLES", c["v"])
    assert planes.shape == (len(c["v"]), 5) and nibbles.shape == (len(c["v"]), 9)
    for v, p, nb, (signs, digits) in zip(c["v"], planes, nibbles, c["want"]):
        sign, d0, d1, d2, top = (int(x) for x in p)
        assert [(sign >> i) & 1 for i in range(64)] + [1] == signs, v
        assert [((d0 >> i) & 1) | (((d1 >> i) & 1) << 1) | (((d2 >> i) & 1) << 2) for i in range(64)] + [top] == digits, v
        want = [sum((digits[8 * k + j] | ((1 - signs[8 * k + j]) << 3)) << (4 * j) for j in range(8)) for k in range(8)]
        assert [int(x) for x in nb[:8]] == want and int(nb[8]) == digits[64], v


def test_one_lane_fused_kernels_read_the_new_digits(eng, monkeypatch):
    """FOURQ_PAIR_MAX=0 on a fresh Engine: 640 elements run one lane per element through the fused kernels (the nibble stream; the planes
    in the constant-time mode)"""
    from fourq_amd import Engine
    c = shared()
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FOURQ_PAIR_MAX", "0")
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        assert np.array_equal(e.mul_endo(c["S"], c["pts"]), c["mul"])
        got, st = e.dh_endo(c["S"], c["aff"])
        assert np.array_equal(st, c["dh"][1]) and not st.any() and np.array_equal(got, c["dh"][0])
        assert np.array_equal(e.mul_endo_mixed(c["S"], c["pts"], c["flags"], c["table"]), c["mixed"])
