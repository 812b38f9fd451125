"""Threshold sharing on the device (fourq_shamir_*, shamir.hip.h) against the fixture tests/golden/shamir.json, the CPU restatement
tests/shamir_ref.py and the library's own grouped sum, in both selection modes.  Every comparison is bit-exact.  The restatement's answers
are computed once per process and shared by both engines.  The neutral point as the result of combine_points is left to the grouped sum's
own tests (the operands would have to be built for it); verify's neutral case is here."""
import functools
import random

import numpy as np
import pytest

import curve4q_oracle as o
import oprf_ref
import shamir_ref as ref
from conftest import load_golden
from fourq_amd import FourQError, _lib, codec

pytestmark = pytest.mark.gpu
N = ref.N
TOP = (1 << 256) - 1
MAX_ID = (1 << 32) - 1
DST = b"FourQ-threshold-OPRF-test"
NOT_ON_CURVE = bytes([2] + [0] * 31)
G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
_combs = {}


def staged(eng):
    """the engine with the generator's comb staged: the calls below pass comb = None"""
    if id(eng) not in _combs:
        _combs[id(eng)] = eng.comb_table(G1_WORDS)
        eng.comb_stage(_combs[id(eng)])
    return eng


def words(values):
    return codec.pack_scalars([int(v) for v in values])


def values(arr):
    return codec.unpack_scalars(np.ascontiguousarray(arr).reshape(-1, 4))


def rows_of(items, width=32):
    return np.frombuffer(b"".join(bytes(b) for b in items), dtype=np.uint8).reshape(len(items), width).copy()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


def dev_full(shape, value=0xAA):
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=torch.uint8, device=torch.device("cuda", 0))


def host(t):
    return t.cpu().numpy()


def u32(ids):
    return np.array(ids, dtype=np.uint32)


# ---- 1. shares --------------------------------------------------------------------------------------------------------------------------
EDGES = [0, 1, N - 1, N, N + 1, TOP]


@functools.lru_cache(maxsize=None)
def polys(n, t):
    """n polynomials of t coefficients: the edge values in every position in turn, random otherwise"""
    rng = random.Random(1000 * n + t)
    out = [[rng.getrandbits(256) for _ in range(t)] for _ in range(n)]
    for r in range(n):
        out[r][r % t] = EDGES[r % len(EDGES)]
        if r % 7 == 3:
            out[r] = [EDGES[(r + j) % len(EDGES)] for j in range(t)]
    return out


@pytest.mark.parametrize("t", [1, 2, 17])
@pytest.mark.parametrize("n,ids", [(3, (1, 2, MAX_ID, 0)), (65, (1, 0, 2, MAX_ID, 2))])
def test_shares_are_the_polynomials_values_party_major(eng, n, ids, t):
    ps = polys(n, t)
    want, want_st = ref.shares(ps, ids)
    coeffs = words([a for p in ps for a in p]).reshape(n, t, 4)
    got, status = eng.shamir_shares(coeffs, u32(ids))
    assert got.shape == (len(ids), n, 4) and status.tolist() == want_st
    flat = values(got)
    for p in range(len(ids)):                                                           # party-major: item (p, r) at index p * n + r
        assert flat[p * n:(p + 1) * n] == want[p], (p, ids[p])
    zero = [p for p, x in enumerate(ids) if x == 0]
    assert zero and all(not got[p].any() and status[p] == _lib.SHAMIR_ID_ZERO for p in zero)
    assert all(v < N for v in flat)


def test_shares_reproduce_the_fixture(eng):
    fx = load_golden("shamir.json", raw=True)
    for p in fx["polys"]:
        coeffs = words(int(a, 16) for a in p["coeffs"]).reshape(1, p["t"], 4)
        got, status = eng.shamir_shares(coeffs, u32(fx["ids"]))
        assert values(got) == [int(s, 16) for s in p["shares"]] and not status.any()


# ---- 2. lagrange ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 3, 16])
def test_lagrange_coefficients_with_differences_of_both_signs(eng, t):
    rng = random.Random(50 + t)
    sets = [[1, MAX_ID, 2, 7, 1000003][:t] if t <= 5 else [1, MAX_ID] + rng.sample(range(2, MAX_ID), t - 2), list(range(t, 0, -1)),
            rng.sample(range(1, MAX_ID), t), [MAX_ID - i for i in range(t)]]
    if t >= 2:
        sets.append([MAX_ID, 1] + rng.sample(range(2, 1 << 20), t - 2))
    got, status = eng.shamir_lagrange(u32(sets))
    assert got.shape == (len(sets), t, 4) and not status.any()
    for s, ids in enumerate(sets):
        lam, _ = ref.lagrange(ids)
        assert values(got[s]) == lam and sum(lam) % N == 1, ids
    if t == 1:
        assert values(got) == [1] * len(sets)


def test_lagrange_300_sets_with_a_zero_and_a_repeat_in_the_middle(eng):
    rng = random.Random(51)
    sets = [rng.sample(range(1, MAX_ID), 3) for _ in range(300)]
    sets[5] = [1, 2, MAX_ID]
    sets[140] = [9, 0, 9]                                                               # the id 0 comes before the repeat
    sets[141] = [0, 3, 4]
    sets[257] = [77, 5, 77]
    got, status = eng.shamir_lagrange(u32(sets))
    want_st = [ref.set_status(ids) for ids in sets]
    assert status.tolist() == want_st
    assert {i: s for i, s in enumerate(want_st) if s} == {140: ref.ID_ZERO, 141: ref.ID_ZERO, 257: ref.ID_REPEATED}
    flat = values(got)
    for s, ids in enumerate(sets):
        assert flat[3 * s:3 * s + 3] == ref.lagrange(ids)[0], (s, ids)
    assert not got[140].any() and not got[141].any() and not got[257].any() and got[139].any(axis=1).all() and got[142].any(axis=1).all()


def test_lagrange_reproduces_the_fixture(eng):
    for s in load_golden("shamir.json", raw=True)["sets"]:
        got, status = eng.shamir_lagrange(u32([s["ids"]]))
        assert values(got) == [int(l, 16) for l in s["lambda"]] and not status.any()


# ---- 3. combine -------------------------------------------------------------------------------------------------------------------------
FIVE = (3, 1, MAX_ID, 9, 4)


@pytest.mark.parametrize("n", [1, 257])
def test_combine_gives_the_secrets_back_from_three_of_five(eng, n):
    ps = polys(n, 3)
    coeffs = words([a for p in ps for a in p]).reshape(n, 3, 4)
    shares, status = eng.shamir_shares(coeffs, u32(FIVE))
    assert not status.any()
    secrets = [p[0] % N for p in ps]
    for pick in ((0, 1, 2), (4, 2, 3)):
        out, st = eng.shamir_combine(u32([FIVE[i] for i in pick]), shares[list(pick)])
        assert st == 0 and values(out) == secrets, pick
    # shares that are not below N are accepted and read modulo N
    lifted = shares[[0, 1, 2]].copy()
    big = [v + N * (((TOP - v) // N) if r % 2 else 1) for r, v in enumerate(values(lifted[1]))]
    lifted[1] = words(big)
    assert all(N <= v <= TOP for v in big)
    out, st = eng.shamir_combine(u32(FIVE[:3]), lifted)
    assert st == 0 and values(out) == secrets
    # two shares of three say nothing
    out, st = eng.shamir_combine(u32(FIVE[:2]), shares[[0, 1]])
    assert st == 0 and values(out) != secrets
    for bad, code in (((3, 0, 4), ref.ID_ZERO), ((3, 4, 3), ref.ID_REPEATED), ((0, 0, 1), ref.ID_ZERO)):
        out, st = eng.shamir_combine(u32(bad), shares[[0, 1, 2]])
        assert st == code and not out.any()


# ---- 4. combine_points ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_scalars(n, t):
    rng = random.Random(4000 + 10 * n + t)
    return [[rng.randrange(1, N) for _ in range(n)] for _ in range(t)]


def points_for(eng, n, t):
    """(t, n, 32) encodings of [k_ir]G and the scalars k: the combination in the exponent is one product on the CPU"""
    k = point_scalars(n, t)
    enc = eng.encode(eng.comb_mul(words([v for block in k for v in block]), _combs[id(staged(eng))])[0])
    return enc.reshape(t, n, 32), k


@pytest.mark.parametrize("n,t", [(1, 1), (3, 5), (257, 3)])
def test_combine_points_is_msm_bytes_over_tiled_and_transposed_operands(eng, n, t):
    ids = [MAX_ID, 1, 6, 2, 77][:t]
    pts, k = points_for(eng, n, t)
    pts = pts.copy()
    bad_row = 2 if n > 2 else None
    if bad_row is not None:
        pts[1, bad_row] = np.frombuffer(NOT_ON_CURVE, dtype=np.uint8)                  # (party 1, row 2) does not decode
    lam, st = eng.shamir_lagrange(u32([ids]))
    assert not st.any()
    out, status = eng.shamir_combine_points(u32(ids), pts)
    want, want_st = eng.msm_bytes(np.tile(lam[0], (n, 1)), pts.transpose(1, 0, 2).reshape(n * t, 32), t)
    assert np.array_equal(out, want) and np.array_equal(status, want_st)
    lam_ref, _ = ref.lagrange(ids)
    assert values(lam) == lam_ref
    gen = o.AffineToR1(o.Gx, o.Gy)
    for r in sorted({0, min(1, n - 1), n // 2, n - 1} - {bad_row}):                                # the CPU's answer on a few rows: [sum lambda_i k_ir]G
        total = sum(l * k[i][r] for i, l in enumerate(lam_ref)) % N
        assert out[r].tobytes() == ref.enc(o.R1toAffine(o.MUL_endo(total, gen))) and status[r] == 0, r
    if bad_row is not None:
        assert status[bad_row] == 16 + _lib.DECODE_NOT_ON_CURVE and not out[bad_row].any()
        assert not np.delete(status, bad_row).any() and np.delete(out, bad_row, axis=0).any(axis=1).all()
        assert ref.combine_points(ids, [[bytes(pts[i, bad_row])] for i in range(t)]) == ([ref.ZERO32], [16 + 2])
    if n == 3:                                                                          # the restatement on whole rows, once
        got_ref = ref.combine_points(ids, [[bytes(b) for b in block] for block in pts])
        assert [bytes(r) for r in out] == got_ref[0] and status.tolist() == got_ref[1]
    if t >= 2:                                                                          # a bad id set comes before the decode codes
        for bad_ids, code in (([0] + ids[1:], ref.ID_ZERO), ([ids[1]] + ids[1:], ref.ID_REPEATED)):
            out, status = eng.shamir_combine_points(u32(bad_ids), pts)
            assert not out.any() and status.tolist() == [code] * n


def test_combine_points_reproduces_the_fixture(eng):
    e = load_golden("shamir.json", raw=True)["exponent"]
    out, status = eng.shamir_combine_points(u32(e["ids"]), rows_of([bytes.fromhex(p) for p in e["points"]]).reshape(3, 1, 32))
    assert out[0].tobytes().hex() == e["combined"] and not status.any()


# ---- 5. end to end: a threshold OPRF is byte for byte the undivided key's --------------------------------------------------------------
def test_threshold_oprf_equals_the_undivided_key(eng):
    rng = random.Random(5)
    key = rng.getrandbits(256)
    msgs = [b"password %d" % i * (i + 1) for i in range(5)]
    matrix, lens = codec.pack_messages(msgs)
    blinds = words(rng.randrange(1, N) for _ in msgs)
    blinded, st = eng.oprf_blind(matrix, blinds, lens, dst=DST)
    assert not st.any()
    coeffs = words([key, rng.randrange(1, N), rng.randrange(1, N)]).reshape(1, 3, 4)
    shares, st = eng.shamir_shares(coeffs, u32(FIVE))
    assert not st.any() and shares.shape == (5, 1, 4)
    want, st = eng.oprf_evaluate(words([key])[0], blinded)
    assert not st.any() and want[0].tobytes() == oprf_ref.evaluate(key, blinded[0].tobytes())[0]
    direct, st = eng.oprf_eval(words([key])[0], matrix, lens, dst=DST)
    assert not st.any()
    for pick in ((0, 1, 2), (4, 2, 3)):
        replies = []
        for i in pick:                                                                  # each server with its share as the key
            z, st = eng.oprf_evaluate(shares[i, 0], blinded)
            assert not st.any() and not np.array_equal(z, want)
            replies.append(z)
        combined, st = eng.shamir_combine_points(u32([FIVE[i] for i in pick]), np.stack(replies))      # party-major as received
        assert not st.any() and np.array_equal(combined, want), pick
        final, st = eng.oprf_finalize(matrix, blinds, combined, lens, dst=DST)
        assert not st.any() and np.array_equal(final, direct)


# ---- 6. verify / public_shares ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dealers():
    """four dealers' polynomials of t = 3 (all coefficients in [1, N)), their commitments by the restatement, and their values at 7"""
    rng = random.Random(6)
    ps = [[rng.randrange(1, N) for _ in range(3)] for _ in range(4)]
    a1, a2 = ps[3][1], ps[3][2]
    ps[3][0] = -(7 * a1 + 49 * a2) % N                                                  # f(7) = 0 mod N: both sides of the check are the neutral point
    assert ps[3][0] != 0
    return ps, [ref.commitments(p) for p in ps], [ref.horner(p, 7) for p in ps]


def test_commitments_are_the_comb_over_the_coefficients(eng):
    staged(eng)
    ps, commits, _ = dealers()
    got = eng.shamir_commitments(words([a for p in ps for a in p]).reshape(4, 3, 4))
    assert got.shape == (4, 3, 32) and [[bytes(c) for c in g] for g in got] == commits
    assert np.array_equal(got, eng.shamir_commitments(words([a for p in ps for a in p]).reshape(4, 3, 4), _combs[id(eng)]))
    zero = eng.shamir_commitments(words([N, 1, 0, 5]).reshape(2, 2, 4))                 # a coefficient that is 0 mod N: the neutral point's encoding
    assert [[bytes(c) for c in g] for g in zero] == [ref.commitments([N, 1]), ref.commitments([0, 5])] and bytes(zero[0, 0]) == ref.NEUTRAL32


def test_public_shares_are_msm_bytes_over_host_made_powers(eng):
    ps, commits, at7 = dealers()
    c32 = rows_of([c for g in commits for c in g]).reshape(4, 3, 32)
    ids = [7, MAX_ID, 1, 7]
    out, status = eng.shamir_public_shares(c32, u32(ids))
    powers = words([pow(x, j, N) for x in ids for j in range(3)])
    want, want_st = eng.msm_bytes(powers, c32.reshape(12, 32), 3)
    assert np.array_equal(out, want) and np.array_equal(status, want_st) and not status.any()
    for g, x in enumerate(ids):
        assert ref.public_share(commits[g], x) == (out[g].tobytes(), 0)
    assert out[3].tobytes() == ref.NEUTRAL32                                            # the neutral point is an ordinary result
    # the id 0 comes before a commitment that does not decode; a refused commitment marks its group only
    bad = c32.copy()
    bad[1, 2] = np.frombuffer(NOT_ON_CURVE, dtype=np.uint8)
    bad[2, 0] = np.frombuffer(ref.NEUTRAL32, dtype=np.uint8)                            # the commitment of a coefficient that is 0 mod N
    out2, status2 = eng.shamir_public_shares(bad, u32([0, 0, 1, 7]))
    assert status2.tolist() == [ref.ID_ZERO, ref.ID_ZERO, ref.REFUSED_NEUTRAL, 0] and not out2[:3].any() and np.array_equal(out2[3], out[3])
    out3, status3 = eng.shamir_public_shares(bad, u32([7, 7, 0, 7]))
    assert status3.tolist() == [0, 16 + _lib.DECODE_NOT_ON_CURVE, ref.ID_ZERO, 0] and np.array_equal(out3[0], out[0]) and not out3[1:3].any()


def test_verify_accepts_honest_shares_and_names_what_is_wrong(eng):
    staged(eng)
    ps, commits, at7 = dealers()
    c32 = rows_of([c for g in commits for c in g]).reshape(4, 3, 32)
    ids = u32([7, 7, 7, 7])
    ok, status = eng.shamir_verify(c32, ids, words(at7))
    assert ok.tolist() == [1, 1, 1, 1] and not status.any() and at7[3] == 0             # group 3: both sides neutral
    assert [ref.verify(commits[g], 7, at7[g]) for g in range(4)] == [(1, 0)] * 4
    shares = words(at7)
    shares[1, 2] ^= np.uint64(1 << 40)                                                  # one flipped bit in a share
    ok, status = eng.shamir_verify(c32, ids, shares)
    assert ok.tolist() == [1, 0, 1, 1] and not status.any()
    swapped = c32.copy()
    swapped[2, [0, 1]] = swapped[2, [1, 0]]                                             # two commitments exchanged
    ok, status = eng.shamir_verify(swapped, ids, words(at7))
    assert ok.tolist() == [1, 1, 0, 1] and not status.any()
    ok, status = eng.shamir_verify(c32, ids, words([at7[0] + N, at7[1], N, at7[3]]))    # a share that is not below N, also the multiple of N
    assert ok.tolist() == [0, 1, 0, 1] and status.tolist() == [_lib.SIG_S_RANGE, 0, _lib.SIG_S_RANGE, 0]
    bad = c32.copy()
    bad[0, 1] = np.frombuffer(NOT_ON_CURVE, dtype=np.uint8)
    ok, status = eng.shamir_verify(bad, u32([7, 0, 7, 7]), words([at7[0], at7[1] + N, at7[2], at7[3]]))
    assert ok.tolist() == [0, 0, 1, 1] and status.tolist() == [16 + _lib.DECODE_NOT_ON_CURVE, ref.ID_ZERO, 0, 0]      # the id 0 before the share's range
    # other recipients: every dealer's share at every id of the fixture's set
    for x in (1, 2, MAX_ID):
        ok, status = eng.shamir_verify(c32, u32([x] * 4), words(ref.horner(p, x) for p in ps))
        assert ok.tolist() == [1, 1, 1, 1] and not status.any()


def test_verify_reproduces_the_fixture(eng):
    staged(eng)
    fx = load_golden("shamir.json", raw=True)
    for p in fx["polys"]:
        c32 = np.tile(rows_of([bytes.fromhex(c) for c in p["commits"]]).reshape(1, p["t"], 32), (4, 1, 1))
        out, status = eng.shamir_public_shares(c32, u32(fx["ids"]))
        assert [r.tobytes().hex() for r in out] == p["public"] and not status.any()
        ok, status = eng.shamir_verify(c32, u32(fx["ids"]), words(int(s, 16) for s in p["shares"]))
        assert ok.tolist() == [1] * 4 and not status.any()


# ---- 7. the argument contract, the reservation, capture ---------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_before_anything_is_touched(eng):
    import ctypes
    staged(eng)
    lib, ctx = eng._lib, eng._ctx
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    ids, sc, pts = u32([1, 2, 3, 4]), np.full((16, 4), 0x55, dtype=np.uint64), np.full((16, 32), 0x55, dtype=np.uint8)
    out, st = np.full((64, 4), 0x77, dtype=np.uint64), np.full(64, 0x77, dtype=np.uint8)
    big = _lib.MAX_BATCH
    calls = {
        "shares": lambda n, t, m=2, null=False: lib.fourq_shamir_shares(ctx, None if null else p(sc), p(ids), p(out), p(st), n, t, m),
        "lagrange": lambda n, t, null=False: lib.fourq_shamir_lagrange(ctx, None if null else p(ids), p(out), p(st), n, t),
        "combine": lambda n, t, null=False: lib.fourq_shamir_combine(ctx, p(ids), None if null else p(sc), p(out), p(st), n, t),
        "combine_points": lambda n, t, null=False: lib.fourq_shamir_combine_points(ctx, p(ids), p(pts), None if null else p(out), p(st), n, t),
        "public_shares": lambda n, t, null=False: lib.fourq_shamir_public_shares(ctx, p(pts), p(ids), p(out), None if null else p(st), n, t),
        "verify": lambda n, t, null=False: lib.fourq_shamir_verify(ctx, None, p(pts), p(ids), None if null else p(sc), p(st), p(st), n, t),
    }
    for name, call in calls.items():
        assert call(0, 3) == _lib.OK, name                                              # nothing to do
        assert call(0, 0) == _lib.OK, name
        assert call(2, 0) == _lib.ERR_INVALID, name                                     # t == 0 with work to do
        assert call(1, _lib.SHAMIR_MAX_T + 1) == _lib.ERR_INVALID, name
        assert call(big // 2, 3) == _lib.ERR_INVALID, name                              # n x t above FOURQ_MAX_BATCH
        assert call(1 << 62, 4) == _lib.ERR_INVALID, name                               # ... and where the product overflows
        assert call(2, 2, null=True) == _lib.ERR_INVALID and call(0, 2, null=True) == _lib.ERR_INVALID, name
    assert calls["shares"](2, 2, m=0) == _lib.OK and calls["shares"](2, 2, m=big) == _lib.ERR_INVALID
    assert lib.fourq_shamir_reserve(ctx, 0, 0) == _lib.OK and lib.fourq_shamir_reserve(ctx, 2, 0) == _lib.ERR_INVALID
    assert lib.fourq_shamir_reserve(ctx, 1, _lib.SHAMIR_MAX_T + 1) == _lib.ERR_INVALID and lib.fourq_shamir_reserve(None, 1, 1) == _lib.ERR_INVALID
    assert (out == 0x77).all() and (st == 0x77).all()
    # the _dev flavours: a misaligned array is refused, ok and status may lie anywhere
    d_ids, d_sc, d_pts, d_out, d_st, d_ok = to_dev(ids), to_dev(sc), to_dev(pts), dev_full((64, 32)), dev_full(64), dev_full(64)
    with pytest.raises(FourQError):
        eng.shamir_shares_dev(d_sc.data_ptr() + 8, d_ids, d_out, d_st, 2, 2, 2)
    with pytest.raises(FourQError):
        eng.shamir_lagrange_dev(d_ids.data_ptr() + 4, d_out, d_st, 1, 3)
    with pytest.raises(FourQError):
        eng.shamir_combine_dev(d_ids, d_sc, d_out.data_ptr() + 8, d_st, 2, 2)
    with pytest.raises(FourQError):
        eng.shamir_combine_points_dev(d_ids, d_pts.data_ptr() + 1, d_out, d_st, 2, 2)
    with pytest.raises(FourQError):
        eng.shamir_public_shares_dev(d_pts, d_ids, d_out.data_ptr() + 8, d_st, 2, 2)
    with pytest.raises(FourQError):
        eng.shamir_verify_dev(d_pts, d_ids, d_sc.data_ptr() + 8, d_ok, d_st, 2, 2)
    eng.sync()
    assert (host(d_out) == 0xAA).all() and (host(d_st) == 0xAA).all() and (host(d_ok) == 0xAA).all()
    ps, commits, at7 = dealers()
    c32 = to_dev(rows_of([c for g in commits for c in g]))
    eng.shamir_verify_dev(c32, to_dev(u32([7, 7, 7, 7])), to_dev(words(at7)), d_ok.data_ptr() + 1, d_st.data_ptr() + 3, 4, 3)
    eng.sync()
    assert host(d_ok)[:6].tolist() == [0xAA, 1, 1, 1, 1, 0xAA] and host(d_st)[:8].tolist() == [0xAA] * 3 + [0] * 4 + [0xAA]


STEPS = ((1, 3), (11, 3), (60, 5))                                                      # (rows, t): 3, 33 and 300 items


def test_dev_calls_on_a_growing_fresh_context_equal_a_reserved_one(eng):
    """as tests/test_gpu_work_hold.py checks its siblings: every _dev call enqueued without a synchronisation on a fresh context, whose outermost
    calls outgrow the work buffer step by step, against a context that fourq_shamir_reserve sized first and that synchronises after every call"""
    import torch
    from fourq_amd import Engine
    comb = _combs[id(staged(eng))]
    rng = random.Random(8)
    rows_top, t_top = STEPS[-1]
    ids_rows = u32([rng.randrange(1, MAX_ID) for _ in range(rows_top)])
    ids_set = u32(rng.sample(range(1, MAX_ID), t_top) + [0] * 3)[:8]
    coeffs = words(rng.randrange(1, N) for _ in range(rows_top * t_top))
    commits = eng.encode(eng.comb_mul(coeffs, comb)[0])
    d_ids_rows, d_ids_set, d_coeffs, d_commits = to_dev(ids_rows), to_dev(ids_set), to_dev(coeffs), to_dev(commits)
    share_steps = []
    for rows, t in STEPS:                                                               # honest shares at each step's shape, one spoiled
        vals = [ref.horner(values(coeffs[g * t:(g + 1) * t]), int(ids_rows[g])) for g in range(rows)]
        vals[rows // 2] ^= 2
        share_steps.append(to_dev(words(vals)))

    def enqueue(e, after):
        outs = []
        for (rows, t), d_shares in zip(STEPS, share_steps):
            sh, st_sh = dev_full((2 * rows, 32)), dev_full(2)
            lam, st_l = dev_full((t, 32)), dev_full(1)
            comb_out, st_c = dev_full((rows, 32)), dev_full(1)
            pts_out, st_p = dev_full((rows, 32)), dev_full(rows)
            pub, st_pub, ok, st_v = dev_full((rows, 32)), dev_full(rows), dev_full(rows), dev_full(rows)
            e.shamir_shares_dev(d_coeffs, d_ids_set, sh, st_sh, rows, t, 2); after()
            e.shamir_lagrange_dev(d_ids_set, lam, st_l, 1, t); after()
            e.shamir_combine_dev(d_ids_set, d_coeffs, comb_out, st_c, rows, t); after()
            e.shamir_combine_points_dev(d_ids_set, d_commits, pts_out, st_p, rows, t); after()
            e.shamir_public_shares_dev(d_commits, d_ids_rows, pub, st_pub, rows, t); after()
            e.shamir_verify_dev(d_commits, d_ids_rows, d_shares, ok, st_v, rows, t); after()
            outs += [sh, st_sh, lam, st_l, comb_out, st_c, pts_out, st_p, pub, st_pub, ok, st_v]
        return outs
    with Engine(0) as fresh, Engine(0) as reserved:
        for e in (fresh, reserved):
            e.ct_select = eng.ct_select
            e.comb_stage(comb)
        reserved.shamir_reserve(rows_top, t_top)
        torch.cuda.synchronize()
        got = enqueue(fresh, lambda: None)
        fresh.sync()
        want = enqueue(reserved, reserved.sync)
        reserved.sync()
        got, want = [host(x) for x in got], [host(x) for x in want]
        torch.cuda.synchronize()
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), [i for i, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]
    for step, (rows, t) in enumerate(STEPS):
        sh, st_sh, lam, st_l, comb_out, st_c, pts_out, st_p, pub, st_pub, ok, st_v = got[12 * step:12 * step + 12]
        assert not st_sh.any() and not st_l.any() and not st_c.any() and not st_p.any() and not st_pub.any() and not st_v.any()
        assert values(lam.view(np.uint64)) == ref.lagrange([int(x) for x in ids_set[:t]])[0]
        expect = np.ones(rows, dtype=np.uint8)
        expect[rows // 2] = 0
        assert np.array_equal(ok, expect) and pts_out.any(axis=1).all() and pub.any(axis=1).all()
        assert np.array_equal(pub, eng.shamir_public_shares(commits[:rows * t].reshape(rows, t, 32), ids_rows[:rows])[0])


def test_dev_calls_can_be_captured_into_a_hip_graph(eng):
    """after shamir_reserve and with the comb staged on the capturing stream the calls only enqueue kernels: one graph deals, checks and
    combines, and a replay over new coefficients in the captured buffers gives the new answers"""
    import torch
    dev = torch.device("cuda", 0)
    ps, commits, at7 = dealers()
    groups, t = 4, 3
    ids = [7, 2, MAX_ID]
    d_coeffs, d_ids = to_dev(words([a for p in ps for a in p])), to_dev(u32(ids + [0]))
    d_commits, d_seven = to_dev(rows_of([c for g in commits for c in g])), to_dev(u32([7] * 4))
    shares, st_s = dev_full((3 * groups, 32)), dev_full(3)
    back, st_b, ok, st_v = dev_full((groups, 32)), dev_full(1), dev_full(groups), dev_full(groups)
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    try:
        eng.comb_stage(eng.comb_table(G1_WORDS))                # staged on this stream, outside the capture
        eng.shamir_reserve(groups, t)
        eng.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            eng.shamir_shares_dev(d_coeffs, d_ids, shares, st_s, groups, t, 3)
            eng.shamir_verify_dev(d_commits, d_seven, shares, ok, st_v, groups, t)          # party 0 of the shares is the id 7
            eng.shamir_combine_dev(d_ids, shares, back, st_b, groups, t)
            graph.capture_end()
        graph.replay()
        torch.cuda.synchronize()
        assert values(host(shares).view(np.uint64)) == [ref.horner(p, x) for x in ids for p in ps] and not host(st_s).any()
        assert host(ok).tolist() == [1] * 4 and not host(st_v).any()
        assert values(host(back).view(np.uint64)) == [p[0] for p in ps] and host(st_b)[0] == 0
        other = [[(a * 3 + 1) % N for a in p] for p in ps]
        d_coeffs.copy_(to_dev(words([a for p in other for a in p])))
        graph.replay()
        torch.cuda.synchronize()
        assert values(host(shares).view(np.uint64)) == [ref.horner(p, x) for x in ids for p in other]
        assert values(host(back).view(np.uint64)) == [p[0] for p in other] and host(ok).tolist() == [0] * 4 and not host(st_v).any()
    finally:
        eng.set_stream(None)
        _combs.pop(id(eng), None)                               # the next test stages the comb again on the engine's own stream


# ---- 8. both selection modes give the same bytes ----------------------------------------------------------------------------------------
_seen = {}


def test_both_selection_modes_give_identical_bytes(eng):
    """combine_points and verify at 3 x 5: whichever mode runs second finds the first one's bytes"""
    staged(eng)
    ids = [MAX_ID, 1, 6, 2, 77]
    pts, _ = points_for(eng, 3, 5)
    out, status = eng.shamir_combine_points(u32(ids), pts)
    rng = random.Random(9)
    polys5 = [[rng.randrange(1, N) for _ in range(5)] for _ in range(3)]
    c32 = eng.shamir_commitments(words([a for p in polys5 for a in p]).reshape(3, 5, 4))
    shares = words(ref.horner(p, x) for p, x in zip(polys5, (7, 2, MAX_ID)))
    shares[1, 0] ^= np.uint64(1)
    pub, st_pub = eng.shamir_public_shares(c32, u32([7, 2, MAX_ID]))
    ok, st_v = eng.shamir_verify(c32, u32([7, 2, MAX_ID]), shares)
    assert ok.tolist() == [1, 0, 1] and not st_v.any() and not status.any() and not st_pub.any()
    got = [a.tobytes() for a in (pts, out, status, c32, pub, ok, st_v)]
    assert _seen.setdefault("bytes", got) == got
