"""The adversarial points and strings (tests/adversarial_points.py) through every entry point that takes or gives the 32-byte wire format:
decode and encode, the projective arrivals of lower_kernel and the R1toAffine primitive, MUL_* and DH_* on bytes on every lane route, and
[k]B + [l]P, the curve part of a verification and the signature check with such strings as keys.

tests/test_adversarial_points.py shows on the CPU what each family is for (a t of decode that is 0 modulo p without being the integer 0,
the x0 == 0 branch of sign(), x in a subfield, y on the limb boundaries of fe_unpack, the refused class and its precedence, points
outside the subgroup) and pins the sources of expectations used here -- oracle/curve4q_oracle.py, oracle_c.encode -- to the real
reference's answers in tests/golden/adversarial_points.json.  Every comparison is bit-exact and covers every row.  Every test takes
`eng`, so everything runs with table selection by address and with constant-time selection; the routes are reached through the
library's test hooks on a fresh Engine, as tests/test_gpu_edge_words.py reaches them."""
import random

import numpy as np
import pytest

import adversarial_points as adv
import curve4q_oracle as o
import oracle_c as oc
import sig_ref as ref
from bench import seeded_scalars
from conftest import load_golden
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu

P = adv.P
M64 = (1 << 64) - 1
G1 = o.AffineToR1(o.Gx, o.Gy)
G1_WORDS = codec.pack_point(G1)
STRINGS = adv.all_strings()
LABELS = ["%s: %s" % (name, label) for name, label, _ in STRINGS]
FAMILY = [name for name, _, _ in STRINGS]
MEMBERS = adv.on_curve_members()
STATUS = {"Malformed point: reserved bit is not zero": _lib.DECODE_RESERVED_BIT, "Point not on curve": _lib.DECODE_NOT_ON_CURVE,
          "type object 'GFp' has no attribute 'two'": _lib.DECODE_REF_ATTRIBUTE_ERROR}
HOOKS = ("FOURQ_PAIR_MAX", "FOURQ_QUAD_MAX", "FOURQ_FUSED_IO")
ROUTE_HOOKS = {"one lane": {"FOURQ_PAIR_MAX": "0"}, "two lanes": {"FOURQ_QUAD_MAX": "0"}, "four lanes": {}}

_cache = {}
POOL = 4093                               # a prime: the two elements of a lane never repeat the same honest row


def rows32(items):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), 32).copy()


def words(rows):
    """rows of GF(p) elements given as integers below 2^128 -> two little-endian words each"""
    return np.array([[w for v in r for w in (v & M64, v >> 64)] for r in rows], dtype=np.uint64)


def lift(aff):
    """AffineToR1 (curve4q.py:100-101) of affine rows: (x, y, 1, x, y)"""
    one = np.zeros((len(aff), 4), dtype=np.uint64)
    one[:, 0] = 1
    return np.hstack([aff, one, aff])


def decode_expectation(strings):
    st, pts = [], []
    for b in strings:
        kind, what = adv.outcome(b)
        st.append(0 if kind == "ok" else STATUS[what])
        pts.append(what if kind == "ok" else ((0, 0), (0, 0)))
    return np.array(st, dtype=np.uint8), codec.pack_points(pts, 2)


def shared():
    """Inputs and expectations, computed once for both selection modes and every route: the Python oracle's decode, the C oracle's
    multiplications.  "mixed": every family row followed by a seeded valid key [m]G, so that neighbours in a wave differ."""
    if _cache:
        return _cache
    c = _cache
    n = len(STRINGS)
    c["raw"] = rows32([b for _, _, b in STRINGS])
    c["st"], c["pts"] = decode_expectation([b for _, _, b in STRINGS])
    assert set(c["st"]) == {0, 1, 2, 3}
    te = oc.table(oc.ENDO, G1_WORDS)
    c["te"] = te
    valid = oc.r1_to_affine(oc.mul(oc.ENDO, seeded_scalars(9901, n), None, te))
    c["mixed_raw"] = np.empty((2 * n, 32), dtype=np.uint8)
    c["mixed_raw"][0::2], c["mixed_raw"][1::2] = c["raw"], oc.encode(valid)
    c["mixed_st"] = np.zeros(2 * n, dtype=np.uint8)
    c["mixed_st"][0::2] = c["st"]
    c["mixed_pts"] = np.empty((2 * n, 8), dtype=np.uint64)
    c["mixed_pts"][0::2], c["mixed_pts"][1::2] = c["pts"], valid
    # scalars: m for the preimages under MUL_*, the fixture's scalar for the rows DH_* was recorded for, seeded ones elsewhere
    c["s_mul"], c["s_dh"] = seeded_scalars(9902, 2 * n), seeded_scalars(9903, 2 * n)
    at = {(name, label): i for i, (name, label, _) in enumerate(STRINGS)}
    c["pre_rows"] = [2 * at["preimages", label] for label, _, _, _ in adv.preimages()]
    for i, (_, _, m, _) in zip(c["pre_rows"], adv.preimages()):
        c["s_mul"][i] = codec.pack_scalars([m])[0]
    c["dh_rows"] = [2 * at[name, label] for name, label, _, _ in adv.dh_rows()]
    for i, (_, _, _, m) in zip(c["dh_rows"], adv.dh_rows()):
        c["s_dh"][i] = codec.pack_scalars([m])[0]
    bad = c["mixed_st"] != 0
    for kind in (oc.ENDO, oc.WINDOWED):
        enc = oc.encode(oc.r1_to_affine(oc.mul(kind, c["s_mul"], lift(c["mixed_pts"]))))
        enc[bad] = 0
        c["mul", kind] = (enc, np.where(bad, 16 + c["mixed_st"], 0).astype(np.uint8))
    g392 = codec.pack_point(o.clear_cofactor(G1))
    for kind in (oc.ENDO, oc.WINDOWED):
        for table in (None, oc.table(kind, g392)):
            out, st = oc.dh(kind, c["s_dh"], c["mixed_pts"], table)
            st = np.where(bad, 16 + c["mixed_st"], st).astype(np.uint8)
            enc = oc.encode(out)
            enc[st != 0] = 0
            c["dh", kind, table is not None] = (enc, st, table)
    return c


def label(i, mixed=True):
    if not mixed:
        return LABELS[i]
    return LABELS[i // 2] if i % 2 == 0 else "the valid key after " + LABELS[i // 2]


def assert_rows(got, want, what, mixed=True):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, (what, len(bad), [label(i, mixed) for i in bad[:6]])


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
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


def dev_empty(shape, dtype):
    import torch
    return torch.empty(shape, dtype=dtype, device=torch.device("cuda", 0))


# ---- decode -----------------------------------------------------------------------------------------------------------------------
def test_decode_every_string(eng):
    import torch
    c = shared()
    for mixed, raw, wst, wpts in ((False, c["raw"], c["st"], c["pts"]), (True, c["mixed_raw"], c["mixed_st"], c["mixed_pts"])):
        out, st = eng.decode(raw)
        assert_rows(st, wst, ("decode status", mixed), mixed)
        assert_rows(out, wpts, ("decode rows", mixed), mixed)        # the point, or a row of zeros where the status is not 0
        assert not out[wst != 0].any()
        d_out, d_st = dev_empty((len(raw), 8), torch.int64), dev_empty(len(raw), torch.uint8)
        eng.decode_dev(to_dev(raw), d_out, d_st, len(raw))
        eng.sync()
        assert_rows(d_st.cpu().numpy(), wst, ("decode_dev status", mixed), mixed)
        assert_rows(d_out.cpu().numpy().view(np.uint64), wpts, ("decode_dev rows", mixed), mixed)
    fam = np.array(FAMILY)
    assert (c["st"][fam == "imaginary_x"] == _lib.DECODE_REF_ATTRIBUTE_ERROR).all() and not c["st"][(fam == "real_x") | (fam == "sign_boundary")].any()


# ---- encode -----------------------------------------------------------------------------------------------------------------------
def twins(points):
    """(name, (n, 8) words) of the same residues: canonical; every half + p; p, then 2p, in place of every half that is 0 (the others
    canonical, then + p); x0 alone + p"""
    rows = [[c for coord in pt for c in coord] for pt in points]
    return [("canonical", words(rows)),
            ("every half + p", words([[v + P for v in r] for r in rows])),
            ("p for 0", words([[v or P for v in r] for r in rows])),
            ("2p for 0, the others + p", words([[v + P if v else 2 * P for v in r] for r in rows])),
            ("x0 + p", words([[r[0] + P] + r[1:] for r in rows])),
            ("x0 + 2p where x0 <= 1", words([[r[0] + (2 * P if r[0] <= 1 else 0)] + r[1:] for r in rows]))]


def test_encode_every_point_and_its_twins(eng):
    import torch
    g = load_golden("adversarial_points.json", raw=True)
    pts = [pt for _, _, pt in MEMBERS]
    names = ["%s: %s" % (name, lb) for name, lb, _ in MEMBERS]
    want = rows32([adv.encode(pt) for pt in pts])
    recorded = [row[0] for name in g["members"] for row in g["members"][name] if isinstance(row, list)]
    assert [bytes(r).hex() for r in want] == recorded                # the reference's own bytes
    zero_x0 = sum(1 for pt in pts if pt[0][0] == 0)
    assert zero_x0 >= len(adv.families()["imaginary_x"])
    for name, w in twins(pts):
        got = eng.encode(w)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, ("encode", name, len(bad), [names[i] for i in bad[:6]])
        out = dev_empty((len(w), 32), torch.uint8)
        eng.encode_dev(to_dev(w), out, len(w))
        eng.sync()
        assert np.array_equal(out.cpu().numpy(), want), ("encode_dev", name)
    wst, wpts = decode_expectation([bytes(r) for r in want])
    out, st = eng.decode(eng.encode(codec.pack_points(pts, 2)))
    assert np.array_equal(st, wst) and np.array_equal(out, wpts)
    assert (wst == _lib.DECODE_REF_ATTRIBUTE_ERROR).sum() >= zero_x0 and (wst == 0).sum() >= 150


# ---- projective arrivals ------------------------------------------------------------------------------------------------------------
def test_projective_arrivals_have_canonical_zeros(eng):
    """R1toAffine of (x z, y z, z) for every point and three kinds of z (seeded, real, imaginary): the affine words, with exact zeros where
    a half of x is 0 modulo p.  Then the preimages: [m]P arrives at S through the ladder's own Z."""
    rng = random.Random(9910)
    pts = [pt for _, _, pt in MEMBERS]
    want = codec.pack_points(pts, 2)
    for kind in ("seeded", "real", "imaginary"):
        rows = []
        for x, y in pts:
            z = {"seeded": (rng.randrange(1, P), rng.randrange(1, P)), "real": (rng.randrange(1, P), 0), "imaginary": (0, rng.randrange(1, P))}[kind]
            X, Y = o.f2_mul(x, z), o.f2_mul(y, z)
            rows.append((X, Y, z, X, Y))
        got = eng.prim("PT_R1TOAFFINE", codec.pack_points(rows, 5))
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (kind, len(bad), [MEMBERS[i][:2] for i in bad[:6]])
    pre = adv.preimages()
    g = load_golden("adversarial_points.json", raw=True)["preimages_mul"]
    p_aff = codec.pack_points([p for _, p, _, _ in pre], 2)
    s_aff = codec.pack_points([s for _, _, _, s in pre], 2)
    ms = codec.pack_scalars([m for _, _, m, _ in pre])
    r1 = oc.mul(oc.WINDOWED, ms, lift(p_aff))
    assert not (r1[:, 8:12] == np.array([1, 0, 0, 0], dtype=np.uint64)).all(axis=1).any()      # no Z is 1
    assert np.array_equal(eng.prim("PT_R1TOAFFINE", r1), s_aff)
    assert np.array_equal(eng.prim("PT_R1TOAFFINE", eng.mul_windowed(ms, lift(p_aff))), s_aff)
    assert np.array_equal(eng.mul_affine(ms, p_aff, kind="windowed"), s_aff)
    endo = eng.mul_affine(ms, p_aff, kind="endo")
    assert np.array_equal(endo, oc.r1_to_affine(oc.mul(oc.ENDO, ms, lift(p_aff))))
    assert ["".join("%032x" % v for coord in pt for v in coord) for pt in codec.unpack_points(endo)] == [row[1] for row in g]
    assert sum(1 for _, _, _, s in pre if s[0][0] == 0) == 6 and sum(1 for _, _, _, s in pre if s[0][1] == 0) == 6


# ---- MUL_* on bytes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_io", ["1", "0"])
@pytest.mark.parametrize("route", list(ROUTE_HOOKS))
def test_mul_bytes_on_every_route(eng, route, fused_io, monkeypatch):
    """every string and a valid key after each, both kinds: decode_kernel in front of the fused one-lane kernels (FOURQ_FUSED_IO=1, one
    lane), decode_lift_kernel everywhere else; lower_kernel<., true> behind them"""
    import torch
    c = shared()
    raw, n = c["mixed_raw"], len(c["mixed_raw"])
    with fresh_engine(eng, dict(ROUTE_HOOKS[route], FOURQ_FUSED_IO=fused_io), monkeypatch) as e:
        for kind_name, kind in (("endo", oc.ENDO), ("windowed", oc.WINDOWED)):
            want, wst = c["mul", kind]
            out, st = e.mul_bytes(c["s_mul"], raw, kind=kind_name)
            assert_rows(st, wst, (route, fused_io, kind_name, "status"))
            assert_rows(out, want, (route, fused_io, kind_name))
            d_out, d_st = dev_empty((n, 32), torch.uint8), dev_empty(n, torch.uint8)
            e.mul_bytes_dev(to_dev(c["s_mul"]), to_dev(raw), d_out, d_st, n, kind=kind_name)
            e.sync()
            assert_rows(d_st.cpu().numpy(), wst, (route, fused_io, kind_name, "dev status"))
            assert_rows(d_out.cpu().numpy(), want, (route, fused_io, kind_name, "dev"))
    want = c["mul", oc.WINDOWED][0]
    for i, (lb, _, _, s) in zip(c["pre_rows"], adv.preimages()):    # [m]P = S: the encoding of a point with a zero half of x
        assert bytes(want[i]) == adv.encode(s), lb


# ---- DH_* on bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTE_HOOKS))
def test_dh_bytes_on_every_route(eng, route, monkeypatch):
    """both kinds, without a table and with the table of [392]G (the key is then decoded and checked only): 16 + the decode status where
    the string does not decode, DH_NEUTRAL for every torsion point that decodes, the oracle's bytes for the rest"""
    import torch
    c = shared()
    raw, n = c["mixed_raw"], len(c["mixed_raw"])
    fam = np.repeat(np.array(FAMILY), 2)
    fam[1::2] = "valid"
    g = load_golden("adversarial_points.json", raw=True)
    with fresh_engine(eng, ROUTE_HOOKS[route], monkeypatch) as e:
        for kind_name, kind in (("endo", oc.ENDO), ("windowed", oc.WINDOWED)):
            for with_table in (False, True):
                want, wst, table = c["dh", kind, with_table]
                out, st = e.dh_bytes(c["s_dh"], raw, kind=kind_name, table=table)
                assert_rows(st, wst, (route, kind_name, with_table, "status"))
                assert_rows(out, want, (route, kind_name, with_table))
                d_out, d_st = dev_empty((n, 32), torch.uint8), dev_empty(n, torch.uint8)
                e.dh_bytes_dev(to_dev(c["s_dh"]), to_dev(raw), table, d_out, d_st, n, kind=kind_name)
                e.sync()
                assert_rows(d_st.cpu().numpy(), wst, (route, kind_name, with_table, "dev status"))
                assert_rows(d_out.cpu().numpy(), want, (route, kind_name, with_table, "dev"))
            want, wst, _ = c["dh", kind, False]
            tors = (fam == "torsion") & (c["mixed_st"] == 0) & np.array(["full order" not in label(i) for i in range(n)])
            assert tors.sum() >= 12 and (wst[tors] == _lib.DH_NEUTRAL).all() and (wst[(fam == "torsion") & ~tors & (c["mixed_st"] == 0)] == 0).all()
            for i, row in zip(c["dh_rows"], g["dh"]):               # the real reference's own outcomes
                cell = row[0 if kind == oc.ENDO else 1]
                if cell.startswith("!"):
                    message = g["_outcomes"][int(cell[1:])][1]
                    assert wst[i] == (_lib.DH_NEUTRAL if "neutral" in message else 16 + STATUS[message]), label(i)
                else:
                    assert wst[i] == 0 and bytes(want[i]).hex() == cell, label(i)


# ---- what a pipeline's own output can be ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTE_HOOKS))
def test_pipelines_emit_subgroup_points_with_a_zero_half(eng, route, monkeypatch):
    """S of the subgroup with x0 = 0 or x1 = 0 as the result of MUL_*(m, P), DH_*(m, Pdh) and [k]G + [l]Pdm (tests/test_adversarial_points.py
    shows that the oracle gets S): canonical words with exact zeros from lower_kernel, normalize_kernel and combine_kernel, and the
    reference's bytes -- the sign from x1 where x0 = 0 -- from lower_kernel<., true>, encode_status_kernel and combine_kernel"""
    rows = adv.subgroup_pipelines() * 40                              # 320 elements: whole waves on every route
    s_aff = codec.pack_points([r[1] for r in rows], 2)
    s_enc = rows32([adv.encode(r[1]) for r in rows])
    m, k, l = (codec.pack_scalars([r[j] for r in rows]) for j in (2, 5, 6))
    p, pdh, pdm = (codec.pack_points([r[j] for r in rows], 2) for j in (3, 4, 7))
    zero = np.zeros(len(rows), dtype=np.uint8)
    assert ((s_aff[:, 0:2] == 0).all(axis=1) | (s_aff[:, 2:4] == 0).all(axis=1)).all()
    with fresh_engine(eng, ROUTE_HOOKS[route], monkeypatch) as e:
        comb = e.comb_table(G1_WORDS)
        for kind in ("endo", "windowed"):
            assert np.array_equal(e.mul_affine(m, p, kind=kind), s_aff), (route, kind)
            out, st = e.mul_bytes(m, oc.encode(p), kind=kind)
            assert np.array_equal(st, zero) and np.array_equal(out, s_enc), (route, kind)
            out, st = (e.dh_endo if kind == "endo" else e.dh_windowed)(m, pdh)
            assert np.array_equal(st, zero) and np.array_equal(out, s_aff), (route, kind)
            out, st = e.dh_bytes(m, oc.encode(pdh), kind=kind)
            assert np.array_equal(st, zero) and np.array_equal(out, s_enc), (route, kind)
        assert np.array_equal(e.double_mul(k, l, pdm, comb), s_aff), route
        out, st = e.double_mul_bytes(k, l, oc.encode(pdm), comb)
        assert np.array_equal(st, zero) and np.array_equal(out, s_enc), route
        ok, st = e.verify_bytes(k, l, oc.encode(pdm), s_enc, comb)
        assert ok.all() and np.array_equal(st, zero), route


# ---- [k]B + [l]P, the curve part of a verification, the signature check ------------------------------------------------------------------
def lane_layout(eng):
    """A device-resident batch beyond two generations shares ONE inversion between the two elements of a lane (combine_kernel<2>: lane t
    owns t and t + T, T = ceil(n / 2)).  Every string is a key twice: at t (its partner t + T an honest key) and at T + M + t (its
    partner M + t an honest key), so each of the two elements of a lane has the failing key in turn.  Honest rows (POOL seeded ones, repeated
    to fill the batch): P = [t]G, expected [(k + l t) mod N]G; the others: the C oracle's two halves joined by the Python oracle's ADD."""
    key = ("layout", eng.lanes)
    if key in _cache:
        return _cache[key]
    c = shared()
    M = len(STRINGS)
    n = 2 * eng.lanes + 131
    T = (n + 1) // 2
    assert 2 * M < T
    placed = np.concatenate([np.arange(M), T + M + np.arange(M)])
    pool = np.arange(n) % POOL                                       # the honest rows: POOL seeded ones, repeated
    k, l, t = seeded_scalars(9921, POOL), seeded_scalars(9922, POOL), seeded_scalars(9923, POOL)
    sums = [(a + b * x) % o.N for a, b, x in zip(codec.unpack_scalars(k), codec.unpack_scalars(l), codec.unpack_scalars(t))]
    keys = oc.encode(oc.r1_to_affine(oc.mul(oc.ENDO, t, None, c["te"])))[pool]
    want = oc.encode(oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, c["te"])))[pool]
    k, l = k[pool], l[pool]
    wst = np.zeros(n, dtype=np.uint8)
    src = np.concatenate([np.arange(M), np.arange(M)])
    keys[placed] = c["raw"][src]
    wst[placed] = np.where(c["st"][src] != 0, _lib.BYTES_DECODE_BASE + c["st"][src], 0)
    want[placed] = joined(c, k[placed], l[placed], c["pts"][src])
    want[wst != 0] = 0
    honest = np.ones(n, dtype=bool)
    honest[placed] = False
    assert honest[placed[:M] + T].all() and honest[placed[M:] - T].all()      # every partner is an honest row
    _cache[key] = {"n": n, "T": T, "M": M, "pool": pool, "placed": placed, "src": src, "k": k, "l": l, "keys": keys, "want": want, "wst": wst, "honest": honest}
    return _cache[key]


def joined(c, k, l, pts):
    """encode([k]G + [l]A) row by row: MUL_endo(k, G) and MUL_endo(l, A) from the C oracle, ADD and R1toAffine from the Python one"""
    first = codec.unpack_points(oc.mul(oc.ENDO, k, None, c["te"]))
    second = codec.unpack_points(oc.mul(oc.ENDO, l, lift(pts)))
    return rows32([adv.encode(o.R1toAffine(o.ADD(a, o.R1toR2(b)))) for a, b in zip(first, second)])


def placed_label(d, i):
    at = np.flatnonzero(d["placed"] == i)
    return "%d: %s" % (i, LABELS[d["src"][at[0]]] if at.size else "an honest key")


def test_double_mul_and_verify_bytes_with_every_string_as_a_key(eng):
    import torch
    d = lane_layout(eng)
    n, k, l, keys, want, wst = d["n"], d["k"], d["l"], d["keys"], d["want"], d["wst"]
    comb = eng.comb_table(G1_WORDS)
    eng.comb_stage(comb)
    out, st = dev_empty((n, 32), torch.uint8), dev_empty(n, torch.uint8)
    eng.double_mul_bytes_dev(to_dev(k), to_dev(l), to_dev(keys), out, st, n)
    eng.sync()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    bad = np.flatnonzero(st != wst)
    assert bad.size == 0, ("status", len(bad), [placed_label(d, i) for i in bad[:6]])
    bad = np.flatnonzero((out != want).any(axis=1))                  # the partners of the failing keys among them: untouched
    assert bad.size == 0, ("rows", len(bad), [placed_label(d, i) for i in bad[:6]])
    assert not out[wst != 0].any() and (wst != 0).sum() == 2 * (shared()["st"] != 0).sum() >= 1000 and {17, 18, 19} <= set(wst)
    # the curve part of a verification: every key that decodes is accepted with the right bytes, torsion keys among them
    expect = want.copy()
    wrong = np.zeros(n, dtype=bool)
    wrong[::9] = True
    expect[wrong, 5] ^= 4
    want_ok = ((wst == 0) & ~wrong).astype(np.uint8)
    ok, st = dev_empty(n, torch.uint8), dev_empty(n, torch.uint8)
    eng.verify_bytes_dev(to_dev(k), to_dev(l), to_dev(keys), to_dev(expect), ok, st, n)
    eng.sync()
    ok, st = ok.cpu().numpy(), st.cpu().numpy()
    bad = np.flatnonzero((ok != want_ok) | (st != wst))
    assert bad.size == 0, ("verify", len(bad), [placed_label(d, i) for i in bad[:6]])
    # host arrays: chunks of one generation, one element per lane (combine_kernel<1>); the rows around the strings
    m = 2 * d["M"] + 77
    out, st = eng.double_mul_bytes(k[:m], l[:m], keys[:m], comb)
    assert np.array_equal(st, wst[:m]) and np.array_equal(out, want[:m])
    ok, st = eng.verify_bytes(k[:m], l[:m], keys[:m], expect[:m], comb)
    assert np.array_equal(ok, want_ok[:m]) and np.array_equal(st, wst[:m])


def sig_layout(eng):
    """the layout above with honest secret keys, messages of 1 to 40 bytes and signatures; every string then takes the place of a key"""
    d = lane_layout(eng)
    c = shared()
    n, placed, src = d["n"], d["placed"], d["src"]
    if "sig" not in d:
        raw = np.random.default_rng(9931).integers(0, 256, size=(POOL, 32), dtype=np.uint8)
        text = np.random.default_rng(9932).integers(0, 256, size=POOL + 64, dtype=np.uint8).tobytes()
        sks, msgs = [r.tobytes() for r in raw], [text[i:i + 1 + i % 40] for i in range(POOL)]
        pks = ref.batch_keygen(sks)
        sigs = ref.batch_sign(sks, pks, msgs)
        matrix, lens = codec.pack_messages(msgs)
        pool = d["pool"]
        pks, sigs, matrix, lens, msgs = pks[pool], sigs[pool], matrix[pool], lens[pool], [msgs[i] for i in pool]
        pks[placed] = c["raw"][src]
        h = codec.pack_scalars([ref.challenge(sigs[i, :32].tobytes(), pks[i].tobytes(), msgs[i]) for i in placed])
        s = np.ascontiguousarray(sigs[placed, 32:]).view("<u8").reshape(-1, 4)
        assert all(v < o.N for v in codec.unpack_scalars(s))
        point = joined(c, s, h, c["pts"][src])
        want_ok = np.ones(n, dtype=np.uint8)
        want_ok[placed] = (point == sigs[placed, :32]).all(axis=1) & (d["wst"][placed] == 0)
        for j in (0, 7, len(placed) - 1):                            # the restatement itself on three of the rows
            i = placed[j]
            assert ref.verify(pks[i].tobytes(), msgs[i], sigs[i].tobytes()) == (want_ok[i], d["wst"][i]), placed_label(d, i)
        d["sig"] = (pks, (matrix, lens), sigs, want_ok)
    return d


def test_sig_verify_with_every_string_as_a_key(eng):
    """honest keys, messages and signatures everywhere; then every string takes the place of a key, twice, as above.  A key that does not
    decode: ok = 0 and FOURQ_BYTES_DECODE_BASE + its status; one that does (a torsion point is a legal key): the restatement's verdict
    on the signature, which was made for another key; every partner stays accepted."""
    import torch
    d = sig_layout(eng)
    n, placed = d["n"], d["placed"]
    pks, (matrix, lens), sigs, want_ok = d["sig"]
    assert want_ok.sum() == n - len(placed)
    eng.comb_stage(eng.comb_table(G1_WORDS))
    ok, st = dev_empty(n, torch.uint8), dev_empty(n, torch.uint8)
    eng.sig_verify_dev(to_dev(pks), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, to_dev(sigs), ok, st, n)
    eng.sync()
    ok, st = ok.cpu().numpy(), st.cpu().numpy()
    bad = np.flatnonzero((ok != want_ok) | (st != d["wst"]))
    assert bad.size == 0, (len(bad), [placed_label(d, i) for i in bad[:6]])
    m = 2 * d["M"] + 77
    ok, st = eng.sig_verify(pks[:m], matrix[:m], sigs[:m], lens[:m])
    assert np.array_equal(ok, want_ok[:m]) and np.array_equal(st, d["wst"][:m])
