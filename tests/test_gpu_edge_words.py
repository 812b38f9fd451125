"""Non-canonical words through the entry points: the ABI accepts any GF(p) element as two words with a value in [0, 2^128)
(include/fourq_amd.h), so fe_unpack hands the bodies top limbs up to 2^24 - 1 where canonical inputs stop at 2^23 - 1.  Every test starts
from canonical inputs, takes the expected result from the C oracle on those, and gives the GPU twins with the same residues: x + p for any
coordinate and x + 2p for x in {0, 1}, chosen per coordinate; for MUL_* (whose formulas need no curve point, as in
test_gpu_mul.py::test_special_base_points) also R1 tuples of extreme words.  Both selection modes (the `eng` fixture); the routes by
size and through the library's test hooks (FOURQ_PAIR_MAX, FOURQ_QUAD_MAX, FOURQ_MIXED_QUEUE, FOURQ_FUSED_IO)."""
import random

import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
from fourq_amd import codec

pytestmark = pytest.mark.gpu

P = (1 << 127) - 1
M64 = (1 << 64) - 1
G1 = o.AffineToR1(o.Gx, o.Gy)
EXTREME = [(1 << 128) - 1, 1 << 127, P, (1 << 127) + (1 << 104) - 1, P - 1, P + 1, 2 * P, 0, 1, (1 << 104) - 1]


def seeded_scalars(seed, n):
    rng = random.Random(seed)
    return np.frombuffer(rng.getrandbits(256 * n).to_bytes(32 * n, "little"), dtype="<u8").reshape(n, 4).copy()


def twin(words, seed):
    """the same residues in non-canonical words: every GF(p) element (two little-endian words) becomes x + p with probability 0.7, and
    x + 2p when x is 0 or 1 with probability 0.5"""
    rng = random.Random(seed)
    w = np.array(words, dtype=np.uint64, copy=True)
    flat = w.reshape(-1, 2)
    for k in range(len(flat)):
        x = int(flat[k, 0]) | int(flat[k, 1]) << 64
        assert x < P
        r = rng.random()
        if x <= 1 and r < 0.5:
            x += 2 * P
        elif r < 0.7:
            x += P
        flat[k, 0], flat[k, 1] = x & M64, x >> 64
    assert not np.array_equal(w, words)
    return w


def affine_to_r1(aff):
    """AffineToR1 (curve4q.py:100-101) of canonical affine rows: (x, y, 1, x, y)"""
    one = np.zeros((len(aff), 4), dtype=np.uint64)
    one[:, 0] = 1
    return np.hstack([aff[:, 0:4], aff[:, 4:8], one, aff[:, 0:4], aff[:, 4:8]])


@pytest.fixture(scope="module")
def data(eng):
    """canonical inputs: projective N-torsion points (raw fixed-base outputs), their affine forms with one off-curve point and one of
    order dividing 392 among them, and G's tables"""
    n = eng.lanes + 300
    sc = seeded_scalars(7101, n)
    pts = eng.mul_endo_fixed(seeded_scalars(7102, n), oc.table(oc.ENDO, codec.pack_point(G1)))
    aff = oc.r1_to_affine(pts[:4000])
    aff[7, 0] ^= 1                                                        # not on the curve
    from conftest import load_golden, unhex
    aff[11] = codec.pack_point(unhex(load_golden("kat.json", raw=True)["P392"]))     # order divides 392
    return {"n": n, "sc": sc, "pts": pts, "aff": aff,
            "te": oc.table(oc.ENDO, codec.pack_point(G1)), "tw": oc.table(oc.WINDOWED, codec.pack_point(G1))}


def _sizes(eng):
    """default routing: four lanes (at most a quarter generation), two lanes (at most half), one-lane fused + a pair tail (past a
    generation)"""
    return (1, 129, eng.lanes // 4, eng.lanes // 4 + 1, eng.lanes // 2 + 1, eng.lanes + 300)


def test_mul_r1_twins_every_route(eng, data):
    sc, pts = data["sc"], data["pts"]
    tw = twin(pts, 1)
    for kind, fn in ((oc.ENDO, eng.mul_endo), (oc.WINDOWED, eng.mul_windowed)):
        want = oc.mul(kind, sc, pts)
        for m in _sizes(eng):
            assert np.array_equal(fn(sc[:m], tw[:m]), want[:m]), (kind, eng.ct_select, m)


def test_mul_extreme_words(eng):
    """R1 tuples whose coordinates are extreme 128-bit words (2^128 - 1, 2^127, p, 2^127 + 2^104 - 1, ...): the oracle's formulas on
    their residues"""
    rng = random.Random(7201)
    tuples = [[rng.choice(EXTREME) for _ in range(10)] for _ in range(12)] + [[w] * 10 for w in EXTREME[:4]]
    words = np.array([[x >> s & M64 for x in t for s in (0, 64)] for t in tuples], dtype=np.uint64)
    ms = [rng.getrandbits(256) for _ in tuples]
    s = codec.pack_scalars(ms)
    red = [tuple((t[2 * k] % P, t[2 * k + 1] % P) for k in range(5)) for t in tuples]
    assert codec.unpack_points(eng.mul_endo(s, words)) == [o.MUL_endo(m, R) for m, R in zip(ms, red)]
    assert codec.unpack_points(eng.mul_windowed(s, words)) == [o.MUL_windowed(m, R) for m, R in zip(ms, red)]


@pytest.mark.parametrize("fused_io", ["1", "0"])
def test_mul_affine_twins(eng, fused_io, monkeypatch):
    """3 * lanes + 77 elements: whole fused generations, where FOURQ_FUSED_IO=1 (the default) hands the ladder affine rows directly and
    =0 goes through the lift kernel and R1 rows, plus a two-lane tail; and 129 elements on the pair kernels"""
    from fourq_amd import Engine
    monkeypatch.setenv("FOURQ_FUSED_IO", fused_io)
    n = 3 * eng.lanes + 77
    sc = seeded_scalars(7151, n)
    aff = oc.r1_to_affine(eng.mul_endo_fixed(seeded_scalars(7152, n), oc.table(oc.ENDO, codec.pack_point(G1))))
    tw = twin(aff, 2)
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        for kind_name, kind in (("endo", oc.ENDO), ("windowed", oc.WINDOWED)):
            want = oc.r1_to_affine(oc.mul(kind, sc, affine_to_r1(aff)))
            for m in (129, n):
                assert np.array_equal(e.mul_affine(sc[:m], tw[:m], kind=kind_name), want[:m]), (kind_name, fused_io, m)


def test_fixed_base_with_non_canonical_tables(eng, data):
    sc = data["sc"][:4000]
    for kind, fn, tab in ((oc.ENDO, eng.mul_endo_fixed, data["te"]), (oc.WINDOWED, eng.mul_windowed_fixed, data["tw"])):
        want = oc.mul(kind, sc, None, tab)
        t2 = twin(tab, 3)
        for m in (1, 129, 4000):
            assert np.array_equal(fn(sc[:m], t2), want[:m]), (kind, m)


def test_mixed_twins(eng, data):
    n = 3000
    sc, pts = data["sc"][:n], data["pts"][:n]
    flags = (seeded_scalars(7301, n)[:, 0] % 3 == 0).astype(np.uint8)
    want = np.where(flags[:, None] == 0, oc.mul(oc.ENDO, sc, None, data["te"]), oc.mul(oc.ENDO, sc, pts))
    got = eng.mul_endo_mixed(sc, twin(pts, 4), flags, twin(data["te"], 5))
    assert np.array_equal(got, want)


def test_dh_twins_keep_every_status(eng, data):
    sc, aff = data["sc"][:4000], data["aff"]
    tw = twin(aff, 6)
    for kind, fn, tab in ((oc.ENDO, eng.dh_endo, data["te"]), (oc.WINDOWED, eng.dh_windowed, data["tw"])):
        want, wst = oc.dh(kind, sc, aff)
        assert wst[7] == 1 and wst[11] == 2
        for m in (12, 129, 4000):
            got, st = fn(sc[:m], tw[:m])
            assert np.array_equal(st, wst[:m]) and np.array_equal(got, want[:m]), (kind, m)
        g = np.repeat(codec.pack_point((o.Gx, o.Gy)).reshape(1, 8), 600, axis=0)
        want, wst = oc.dh(kind, sc[:600], g, tab)
        got, st = fn(sc[:600], twin(g, 7), twin(tab, 8))
        assert not st.any() and not wst.any() and np.array_equal(got, want), kind


def test_dh_exchange_twins(eng, data):
    n = 600
    a, b = seeded_scalars(7401, n), seeded_scalars(7402, n)
    G = (o.Gx, o.Gy)
    g = np.repeat(codec.pack_point(G).reshape(1, 8), n, axis=0)
    mid, s1 = oc.dh(oc.ENDO, b, g)
    want, s2 = oc.dh(oc.ENDO, a, mid)
    assert not s1.any() and not s2.any()
    base = twin(codec.pack_point(G).reshape(1, 8), 9).ravel()
    out, st = eng.dh_exchange(a, b, base)
    assert not st.any() and np.array_equal(out, want)
    t392 = twin(oc.table(oc.ENDO, codec.pack_point(o.MUL_endo(392, G1))), 10)
    out, st = eng.dh_exchange(a, b, base, table392=t392)
    assert not st.any() and np.array_equal(out, want)


def test_tables_comb_and_encode_of_twins(eng, data):
    pts = data["pts"][:8]
    for k in range(8):
        Pt = pts[k]
        tw = twin(Pt, 20 + k)
        assert np.array_equal(eng.table_endo(tw), oc.table(oc.ENDO, Pt)), k
        assert np.array_equal(eng.table_windowed(tw), oc.table(oc.WINDOWED, Pt)), k
    B = codec.pack_point(o.MUL_endo(392, G1))
    comb = eng.comb_table(B)
    comb_tw = eng.comb_table(twin(B, 30))
    assert np.array_equal(comb_tw, comb)
    s = seeded_scalars(7501, 700)
    g = np.repeat(codec.pack_point((o.Gx, o.Gy)).reshape(1, 8), 700, axis=0)
    want, wst = oc.dh(oc.ENDO, s, g)
    got, st = eng.comb_mul(s, comb_tw)
    assert not st.any() and np.array_equal(got, want)
    aff = oc.r1_to_affine(data["pts"][:3000])
    assert np.array_equal(eng.encode(twin(aff, 31)), oc.encode(aff))


ROUTE_HOOKS = {"one lane": {"FOURQ_PAIR_MAX": "0"}, "two lanes": {"FOURQ_QUAD_MAX": "0"}, "four lanes": {}}


@pytest.mark.parametrize("hook", list(ROUTE_HOOKS))
def test_every_entry_point_on_the_hooked_routes(eng, data, hook, monkeypatch):
    """1 500 elements with FOURQ_PAIR_MAX=0: the one-lane fused kernels (variable base, DH's load_fe2 -> cofactor clearing -> fused table
    build) and the LDS ladders (fixed base); FOURQ_QUAD_MAX=0: the two-lane kernels; by default: four lanes.  MUL_*, affine MUL_*, fixed
    base, DH with and without a table (statuses kept), mixed batches -- every input in non-canonical words."""
    from fourq_amd import Engine
    for k in ("FOURQ_PAIR_MAX", "FOURQ_QUAD_MAX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTE_HOOKS[hook].items():
        monkeypatch.setenv(k, v)
    m = 1500
    sc, pts, aff = data["sc"][:m], data["pts"][:m], data["aff"][:m]
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        for kind, fn in ((oc.ENDO, e.mul_endo), (oc.WINDOWED, e.mul_windowed)):
            assert np.array_equal(fn(sc, twin(pts, 50)), oc.mul(kind, sc, pts)), (hook, kind)
        caff = oc.r1_to_affine(pts)
        for kind_name, kind in (("endo", oc.ENDO), ("windowed", oc.WINDOWED)):
            want = oc.r1_to_affine(oc.mul(kind, sc, affine_to_r1(caff)))
            assert np.array_equal(e.mul_affine(sc, twin(caff, 51), kind=kind_name), want), (hook, kind_name)
        for kind, fn, tab in ((oc.ENDO, e.mul_endo_fixed, data["te"]), (oc.WINDOWED, e.mul_windowed_fixed, data["tw"])):
            assert np.array_equal(fn(sc, twin(tab, 52)), oc.mul(kind, sc, None, tab)), (hook, kind)
        g = np.repeat(codec.pack_point((o.Gx, o.Gy)).reshape(1, 8), m, axis=0)
        for kind, fn, tab in ((oc.ENDO, e.dh_endo, data["te"]), (oc.WINDOWED, e.dh_windowed, data["tw"])):
            want, wst = oc.dh(kind, sc, aff)
            got, st = fn(sc, twin(aff, 53))
            assert wst[7] == 1 and wst[11] == 2 and np.array_equal(st, wst) and np.array_equal(got, want), (hook, kind)
            want, wst = oc.dh(kind, sc, g, tab)
            got, st = fn(sc, twin(g, 54), twin(tab, 55))
            assert not wst.any() and np.array_equal(st, wst) and np.array_equal(got, want), (hook, kind, "table")
        flags = (seeded_scalars(7302, m)[:, 0] % 3 == 0).astype(np.uint8)
        want = np.where(flags[:, None] == 0, oc.mul(oc.ENDO, sc, None, data["te"]), oc.mul(oc.ENDO, sc, pts))
        assert np.array_equal(e.mul_endo_mixed(sc, twin(pts, 56), flags, twin(data["te"], 57)), want), hook


@pytest.mark.parametrize("queue", ["0", "1"])
def test_mixed_routes_twins(eng, data, queue, monkeypatch):
    """FOURQ_MIXED_QUEUE=0: the three launches of a mixed batch; =1: the persistent work-queue kernel (9 001 elements)"""
    from fourq_amd import Engine
    monkeypatch.setenv("FOURQ_MIXED_QUEUE", queue)
    m = 9001
    sc, pts = data["sc"][:m], data["pts"][:m]
    flags = (seeded_scalars(7303, m)[:, 0] % 3 == 0).astype(np.uint8)
    want = np.where(flags[:, None] == 0, oc.mul(oc.ENDO, sc, None, data["te"]), oc.mul(oc.ENDO, sc, pts))
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        assert np.array_equal(e.mul_endo_mixed(sc, twin(pts, 58), flags, twin(data["te"], 59)), want), queue


def test_constant_time_mixed_tail_twins(data):
    """constant-time mode, lanes + 300 variable-base ids and 3 000 fixed-base ones: the ids past the whole fused generation ride with
    the fixed-base elements in mixed_ct_tail_kernel (test_gpu_mul.py::test_constant_time_mixed_round_cuts_a_small_remainder_off...)"""
    from fourq_amd import Engine
    with Engine(0) as e:
        e.ct_select = True
        n_var, n_fix = e.lanes + 300, 3000
        n = n_var + n_fix
        flags = np.ones(n, dtype=np.uint8)
        flags[np.random.RandomState(71).choice(n, n_fix, replace=False)] = 0
        sc = seeded_scalars(7304, n)
        pts = e.mul_endo_fixed(seeded_scalars(7305, n), data["te"])
        want = oc.mul(oc.ENDO, sc, pts)
        fix = np.flatnonzero(flags == 0)
        want[fix] = oc.mul(oc.ENDO, sc[fix], None, data["te"])
        assert np.array_equal(e.mul_endo_mixed(sc, twin(pts, 60), flags, twin(data["te"], 61)), want)
