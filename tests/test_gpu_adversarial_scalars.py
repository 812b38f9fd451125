"""The adversarial scalar families (tests/adversarial_scalars.py) through the device's integer code on every route that compiles it in:
the primitives, the variable- and fixed-base ladders with four, two and one lane per element, the mixed
batches, DH, the comb's three kernels in both shapes, its deferred flavour under [k]B + [l]P, and the exchange.

tests/test_adversarial_scalars.py shows on the CPU what each family is for (the last rounds of comb_recode's plane iteration, the floor
of mul_shift256's truncated product, the second comparisons of win_reduce's borrow and carry chains, ge256 on operands that agree from
the top, Barrett's quotient) and pins every source of expectations used here -- tests/golden/adversarial.json (the real reference),
oracle/curve4q_oracle.py, oracle/fourq_oracle.c and Python integers -- against each other.  Every test takes `eng`, so everything
runs with table selection by address and with constant-time selection; the routes are reached through the library's test hooks on a
fresh Engine, as tests/test_gpu_edge_words.py reaches them."""
import numpy as np
import pytest

import adversarial_scalars as adv
import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_scalars
from conftest import load_golden
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu

N = o.N
G1 = o.AffineToR1(o.Gx, o.Gy)
G1_WORDS = codec.pack_point(G1)
G_AFF = codec.pack_point((o.Gx, o.Gy))
FAM = adv.families256()
MS = [m for _, m in FAM]
PAD = 640                                 # every batch: the families and seeded padding up to this many elements (several blocks of every kernel)
HOOKS = ("FOURQ_PAIR_MAX", "FOURQ_QUAD_MAX", "FOURQ_MIXED_QUEUE")
LADDER_ROUTES = {"four lanes": {}, "two lanes": {"FOURQ_QUAD_MAX": "0"}, "one lane": {"FOURQ_PAIR_MAX": "0"}}
COMB_ROUTES = LADDER_ROUTES

_cache = {}


def shared():
    """Inputs and expectations, computed once for both selection modes and every route: all of it from the C oracle and Python integers."""
    if _cache:
        return _cache
    c = _cache
    assert len(MS) < PAD
    c["S"] = np.vstack([codec.pack_scalars(MS), seeded_scalars(8801, PAD - len(MS))])
    c["ms"] = codec.unpack_scalars(c["S"])
    n = PAD
    te, tw = oc.table(oc.ENDO, G1_WORDS), oc.table(oc.WINDOWED, G1_WORDS)
    c["table"] = {oc.ENDO: te, oc.WINDOWED: tw}
    q = oc.mul(oc.ENDO, seeded_scalars(8802, 1), None, te)[0]            # a seeded point of order N, projective (Z != 1)
    c["points"] = {"G": np.repeat(G1_WORDS.reshape(1, 20), n, axis=0), "Q": np.repeat(q.reshape(1, 20), n, axis=0)}
    c["affine"] = {"G": np.repeat(G_AFF.reshape(1, 8), n, axis=0), "Q": np.repeat(oc.r1_to_affine(q.reshape(1, 20)), n, axis=0)}
    g392 = codec.pack_point(o.clear_cofactor(G1))
    c["table392"] = {kind: oc.table(kind, g392) for kind in (oc.ENDO, oc.WINDOWED)}
    for kind in (oc.ENDO, oc.WINDOWED):
        for b in ("G", "Q"):
            c["mul", kind, b] = oc.mul(kind, c["S"], c["points"][b])
            c["dh", kind, b] = oc.dh(kind, c["S"], c["affine"][b])
        c["fixed", kind] = oc.mul(kind, c["S"], None, c["table"][kind])
        c["dh", kind, "table"] = oc.dh(kind, c["S"], c["affine"]["G"], c["table392"][kind])
        assert np.array_equal(c["dh", kind, "table"][0], c["dh", kind, "G"][0])
    c["flags"] = (np.arange(n) % 2).astype(np.uint8)
    return c


def fresh_engine(eng, hooks, monkeypatch):
    from fourq_amd import Engine
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in hooks.items():
        monkeypatch.setenv(k, v)
    e = Engine(0)
    e.ct_select = eng.ct_select
    return e


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def dev_empty(shape, dtype):
    import torch
    return torch.empty(shape, dtype=dtype, device=torch.device("cuda", 0))


def bad_rows(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))


def label(i):
    return FAM[i][0] if i < len(FAM) else "padding %d" % i


def assert_rows(got, want, what):
    bad = bad_rows(got, want)
    assert bad.size == 0, (what, len(bad), [label(i) for i in bad[:6]])


# ---- primitives -------------------------------------------------------------------------------------------------------------------
def test_recoding_primitives(eng):
    c = shared()
    S, ms = c["S"], c["ms"]
    dec = eng.prim("SC_DECOMPOSE", S)
    assert_rows(dec, np.array([o.decompose(m) for m in ms], dtype=np.uint64), "decompose")
    rec = eng.prim("SC_RECODE", dec)
    win = eng.prim("SC_WINDOWED", S)
    want_rec, want_win = [], []
    for m in ms:
        signs, digits = o.recode(o.decompose(m))
        planes = [sum(((d >> b) & 1) << i for i, d in enumerate(digits[:64])) for b in range(3)]
        want_rec.append([sum(s << i for i, s in enumerate(signs[:64]))] + planes + [digits[64]])
        sgn, ind = o.recode_windowed(m)
        want_win.append(bytes((s << 3) | i for s, i in zip(sgn, ind)))
    assert_rows(rec, np.array(want_rec, dtype=np.uint64), "recode")
    assert_rows(np.array([np.frombuffer(r.tobytes()[:63], dtype=np.uint8) for r in win]),
                np.array([np.frombuffer(w, dtype=np.uint8) for w in want_win]), "fixed-window digits")
    # the real reference's own answers, row by row
    rows = load_golden("adversarial.json", raw=True)["rows"]
    order = [i for i, (lb, _) in enumerate(FAM) if not adv.is_seeded(lb)] + [i for i, (lb, _) in enumerate(FAM) if adv.is_seeded(lb)]
    assert sum(1 for lb, _ in FAM if not adv.is_seeded(lb)) <= len(rows) <= len(order)
    for i, r in zip(order, rows):                                   # row by row in the fixture's order: the constructed members, then the seeded ones
        assert [int(x) for x in dec[i]] == [int(r[0][16 * j:16 * j + 16], 16) for j in range(4)], label(i)
        sign, d0, d1, d2, top = (int(x) for x in rec[i])
        assert sign | (1 << 64) == int(r[1], 16), label(i)
        assert "".join(str(((d0 >> j) & 1) | (((d1 >> j) & 1) << 1) | (((d2 >> j) & 1) << 2)) for j in range(64)) + str(top) == r[2], label(i)
        assert "".join("%x" % b for b in win[i].tobytes()[:63]) == r[3], label(i)


def rows_words(rows, widths):
    return np.array([sum((adv.words(v, w) for v, w in zip(r, widths)), []) for r in rows], dtype=np.uint64)


def values(out):
    return [adv.from_words([int(w) for w in r]) for r in out]


def test_arithmetic_modulo_n(eng):
    xs = [x for _, x in adv.barrett_boundary()] + MS
    got = values(eng.prim("SC_REDUCE512", rows_words([(x,) for x in xs], (8,))))
    bad = [hex(x) for g, x in zip(got, xs) if g != x % N]
    assert not bad, bad[:4]
    consts = (1, N - 1, N, (1 << 256) - 1)
    # Barrett's boundary goes in through SC_REDUCE512 above; the 256-bit families through either operand here, against {1, N - 1, N, 2^256 - 1}
    # and against each other
    rows = [(a, b) for v in MS for cst in consts for a, b in ((v, cst), (cst, v))] + [(v, w) for v, w in zip(MS, MS[1:] + MS[:1])]
    got = values(eng.prim("SC_MUL", rows_words(rows, (4, 4))))
    bad = [tuple(map(hex, r)) for g, r in zip(got, rows) if g != r[0] * r[1] % N]
    assert not bad, bad[:4]
    rows = []
    for v in MS:
        for j, cst in enumerate(consts):
            other = consts[(j + 1) % 4]
            rows += [(v, cst, other), (cst, v, other), (other, cst, v)]
    rows += [(u, v, w) for u, v, w in zip(MS, MS[1:] + MS[:1], MS[2:] + MS[:2])]
    got = values(eng.prim("SC_MULSUB", rows_words(rows, (4, 4, 4))))
    bad = [tuple(map(hex, r)) for g, r in zip(got, rows) if g != (r[0] - r[1] * r[2]) % N]
    assert not bad, bad[:4]


# ---- ladders ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(LADDER_ROUTES))
def test_ladders_on_every_route(eng, route, monkeypatch):
    """MUL_* on G and on a seeded point, fixed base, mixed batches with either flag on every scalar, DH with and without a table."""
    c = shared()
    S = c["S"]
    with fresh_engine(eng, LADDER_ROUTES[route], monkeypatch) as e:
        for kind, name, mul, fixed, dh in ((oc.ENDO, "endo", e.mul_endo, e.mul_endo_fixed, e.dh_endo),
                                           (oc.WINDOWED, "windowed", e.mul_windowed, e.mul_windowed_fixed, e.dh_windowed)):
            for b in ("G", "Q"):
                assert_rows(mul(S, c["points"][b]), c["mul", kind, b], (route, "mul", name, b))
                want, wst = c["dh", kind, b]
                got, st = dh(S, c["affine"][b])
                assert np.array_equal(st, wst), (route, "dh", name, b, [label(i) for i in np.flatnonzero(st != wst)[:6]])
                assert_rows(got, want, (route, "dh", name, b))
            assert_rows(fixed(S, c["table"][kind]), c["fixed", kind], (route, "fixed", name))
            want, wst = c["dh", kind, "table"]
            got, st = dh(S, c["affine"]["G"], c["table392"][kind])
            assert np.array_equal(st, wst) and (wst == _lib.DH_NEUTRAL).sum() >= 11, (route, "dh table", name)
            assert_rows(got, want, (route, "dh table", name))
        for flags in (c["flags"], 1 - c["flags"]):
            want = np.where(flags[:, None] == 0, c["fixed", oc.ENDO], c["mul", oc.ENDO, "Q"])
            assert_rows(e.mul_endo_mixed(S, c["points"]["Q"], flags, c["table"][oc.ENDO]), want, (route, "mixed"))


@pytest.mark.parametrize("queue", ["0", "1"])
def test_mixed_batches_with_and_without_the_work_queue(eng, queue, monkeypatch):
    c = shared()
    with fresh_engine(eng, {"FOURQ_MIXED_QUEUE": queue}, monkeypatch) as e:
        for flags in (c["flags"], 1 - c["flags"]):
            want = np.where(flags[:, None] == 0, c["fixed", oc.ENDO], c["mul", oc.ENDO, "Q"])
            assert_rows(e.mul_endo_mixed(c["S"], c["points"]["Q"], flags, c["table"][oc.ENDO]), want, ("mixed queue", queue))


def test_ladder_device_flavour_equals_the_host_one(eng):
    import torch
    c = shared()
    out = dev_empty((PAD, 20), torch.int64)
    eng.mul_endo_dev(to_dev(c["S"]), to_dev(c["points"]["Q"]), out, PAD)
    eng.sync()
    got = out.cpu().numpy().view(np.uint64)
    assert_rows(got, c["mul", oc.ENDO, "Q"], "mul_endo_dev")
    assert np.array_equal(got, eng.mul_endo(c["S"], c["points"]["Q"]))


# ---- comb -------------------------------------------------------------------------------------------------------------------------
def comb_expectation(name):
    """R1toAffine(MUL_endo(m, B)) with comb_mul's conventions: the neutral point is status DH_NEUTRAL and a row of zeros"""
    c = shared()
    if ("comb", name) not in c:
        B = G1 if name == "G" else o.MUL_endo(392, G1)
        want = oc.r1_to_affine(oc.mul(oc.ENDO, c["S"], None, oc.table(oc.ENDO, codec.pack_point(B))))
        neutral = np.array([m % N == 0 for m in c["ms"]])
        assert np.array_equal(neutral, (want == codec.pack_point((o.Ox, o.Oy))).all(axis=1)) and neutral.sum() >= 11
        want[neutral] = 0
        c["comb", name] = (codec.pack_point(B), want, np.where(neutral, _lib.DH_NEUTRAL, 0).astype(np.uint8))
    return c["comb", name]


@pytest.mark.parametrize("route", list(COMB_ROUTES))
def test_comb_on_every_kernel(eng, route, monkeypatch):
    """comb_quad_kernel<., 4>, <., 2> and the one-lane comb_kernel; the selection mode decides the shape (1 024 or 80 points), and each
    shape finds its own comb_ripple family among the scalars"""
    c = shared()
    with fresh_engine(eng, COMB_ROUTES[route], monkeypatch) as e:
        for name in ("G", "[392]G"):
            B, want, wst = comb_expectation(name)
            got, st = e.comb_mul(c["S"], e.comb_table(B))
            assert np.array_equal(st, wst), (route, name, [label(i) for i in np.flatnonzero(st != wst)[:6]])
            assert_rows(got, want, (route, "comb", name))


def test_comb_device_flavour_equals_the_host_one(eng):
    import torch
    c = shared()
    B, want, wst = comb_expectation("[392]G")
    comb = eng.comb_table(B)
    out, st = dev_empty((PAD, 8), torch.int64), dev_empty(PAD, torch.uint8)
    eng.comb_mul_dev(to_dev(c["S"]), comb, out, st, PAD)
    eng.sync()
    got, got_st = out.cpu().numpy().view(np.uint64), st.cpu().numpy()
    assert np.array_equal(got_st, wst)
    assert_rows(got, want, "comb_mul_dev")
    host, host_st = eng.comb_mul(c["S"], comb)
    assert np.array_equal(got, host) and np.array_equal(got_st, host_st)


def double_mul_expectation():
    """[k]G + [l][t]G = [(k + l t) mod N]G: the modular arithmetic in Python integers, the points from the C oracle.  The adversarial
    scalars as k against seeded l, and as l against seeded k."""
    c = shared()
    if "double" not in c:
        te = c["table"][oc.ENDO]
        other, t = seeded_scalars(8803, PAD), seeded_scalars(8804, PAD)
        P = oc.r1_to_affine(oc.mul(oc.ENDO, t, None, te))
        cases = []
        for k, l in ((c["S"], other), (other, c["S"])):
            sums = [(a + b * x) % N for a, b, x in zip(codec.unpack_scalars(k), codec.unpack_scalars(l), codec.unpack_scalars(t))]
            cases.append((k, l, oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, te))))
        c["double"] = (P, cases)
    return c["double"]


@pytest.mark.parametrize("route", ["four lanes", "one lane"])
def test_deferred_comb_under_double_mul(eng, route, monkeypatch):
    """comb_kernel's deferred flavour (projective output) with the variable half on the four-lane kernels and on the fused one-lane ones"""
    import torch
    P, cases = double_mul_expectation()
    with fresh_engine(eng, COMB_ROUTES[route], monkeypatch) as e:
        comb = e.comb_table(G1_WORDS)
        for which, (k, l, want) in zip(("as k", "as l"), cases):
            got = e.double_mul(k, l, P, comb)
            assert_rows(got, want, (route, "double_mul", which))
            out = dev_empty((PAD, 8), torch.int64)
            e.double_mul_dev(to_dev(k), to_dev(l), to_dev(P), out, PAD, comb_host=comb)
            e.sync()
            assert np.array_equal(out.cpu().numpy().view(np.uint64), got), (route, "double_mul_dev", which)


def test_exchange_with_adversarial_key_generation(eng):
    c = shared()
    a, b = seeded_scalars(8805, PAD), c["S"]
    mid, s1 = c["dh", oc.ENDO, "G"]
    want, s2 = oc.dh(oc.ENDO, a, mid)
    ws = np.where(s1 != 0, s1, s2)
    want[ws != 0] = 0
    assert (ws == _lib.DH_NEUTRAL).sum() >= 11 and (ws == 0).sum() >= PAD - 40
    out, st = eng.dh_exchange_comb(a, b, eng.comb_table(codec.pack_point(o.MUL_endo(392, G1))))
    assert np.array_equal(st, ws), [label(i) for i in np.flatnonzero(st != ws)[:6]]
    assert_rows(out, want, "dh_exchange_comb")
