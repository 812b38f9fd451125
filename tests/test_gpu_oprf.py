"""The oblivious PRF on the device (fourq_oprf_* / fourq_scalar_inv_*, oprf.hip.h and scalar_n.hip.h's sc_inv) against Python's pow,
the CPU restatement tests/oprf_ref.py, the fixture tests/golden/oprf.json and -- for the large shapes -- the composition of calls that
other test files already pin (hash_to_curve, mul_affine, encode, dh_bytes, mul_bytes, sha512), in both selection modes.  The restatement's
answers are computed once per process and shared by both engines."""
import functools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import adversarial_scalars as advs
import oprf_ref as ref
from fourq_amd import FourQError, _lib, codec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = ref.N
TOP = (1 << 256) - 1
DST = b"FourQ-OPRF-V01-test"
SIZES = (1, 63, 64, 65, 257)
SHIPPED_K = (1, 8, 16)


def rows_of(items, width):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), width).copy()


def bad_rows(got, expect):
    got, expect = np.asarray(got).reshape(len(expect), -1), np.asarray(expect).reshape(len(expect), -1)
    return np.flatnonzero((got != expect).any(axis=1))


def inv_words(values):
    return codec.pack_scalars([pow(v % N, -1, N) if v % N else 0 for v in values])


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


def dev_empty(shape, dtype):
    import torch
    return torch.empty(shape, dtype=dtype, device=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def batch():
    """257 rows of mixed lengths 0 .. 150 in strides 160 and 163 (the same messages), blinds (some above N), one key, and the
    restatement's blinded / evaluated elements and outputs."""
    rng = random.Random(20261019)
    n = SIZES[-1]
    lens = np.array([rng.randrange(151) for _ in range(n)], dtype=np.uint32)
    lens[:8] = (0, 1, 69, 70, 86, 87, 150, 16)                   # F's string with this DST: 60 + len bytes; 111 | 112 and 127 | 128 | 129 at 51 / 52 and 67 .. 69
    lens[8:13] = (51, 52, 67, 68, 69)
    wide = np.random.default_rng(12).integers(0, 256, size=(n, 163), dtype=np.uint8)
    blinds = [rng.randrange(1, N) + (N if i % 5 == 0 else 0) for i in range(n)]
    key = rng.getrandbits(256)
    msgs = [wide[i, :lens[i]].tobytes() for i in range(n)]
    blinded = [ref.blind(m, DST, r)[0] for m, r in zip(msgs, blinds)]
    evaluated = [ref.evaluate(key, b)[0] for b in blinded]
    output = [ref.evaluate_direct(key, m, DST)[0] for m in msgs]
    assert all(ref.finalize(m, DST, r, z) == (out, 0) for m, r, z, out in list(zip(msgs, blinds, evaluated, output))[:8])
    return {"m160": np.ascontiguousarray(wide[:, :160]), "m163": wide, "lens": lens, "blinds": blinds, "r": codec.pack_scalars(blinds), "key": key,
            "k": codec.pack_scalars([key])[0], "blinded": rows_of(blinded, 32), "evaluated": rows_of(evaluated, 32), "output": rows_of(output, 64)}


def fresh_engine(eng, scinv_group):
    """an engine of its own with K forced (fourq_ctx_set_scinv_group, a test hook behind FOURQ_DEBUG_ROUTES=1, which conftest.py sets)"""
    from fourq_amd import Engine
    e = Engine(0)
    e.ct_select = eng.ct_select
    e.set_scinv_group(scinv_group)
    return e


# ---- 1. the inversion modulo N ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inversion_inputs():
    rng = random.Random(71)
    special = [0, 1, 2, N - 1, N, N + 1, 2 * N, TOP, (N + 1) // 2, (N - 1) // 2]
    values = special + [m for _, m in advs.families256()] + [rng.getrandbits(256) for _ in range(2000)]
    return values, codec.pack_scalars(values), inv_words(values)


def test_scalar_inv_against_pow(eng):
    values, words, want = inversion_inputs()
    assert len(values) > 2000 and (want[[0, 4, 6]] == 0).all() and want[1, 0] == 1       # 0, N, 2N -> 0; 1 -> 1
    for label, got in (("primitive", eng.prim("SC_INV", words)), ("scalar_inv", eng.scalar_inv(words))):
        assert bad_rows(got, want).size == 0, (label, bad_rows(got, want)[:8])
    # x * (1 / x) = 1 through the library's own product, for every unit
    units = np.array([v % N != 0 for v in values])
    prod = eng.prim("SC_MUL", np.hstack([words, want]))
    assert (prod[units] == np.array([1, 0, 0, 0], dtype=np.uint64)).all()
    assert eng.scalar_inv(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)


def test_scalar_inv_batch_sizes_and_the_device_form(eng):
    import torch
    _, words, want = inversion_inputs()
    for n in (1, 7, 8, 9, 63, 64, 65, 257):
        got = eng.scalar_inv(words[10:10 + n])
        assert bad_rows(got, want[10:10 + n]).size == 0, n
    n = 2 * eng.lanes + 1                                           # past one wave per SIMD: several elements per inversion
    reps = -(-n // len(words))
    big, big_want = np.tile(words, (reps, 1))[:n], np.tile(want, (reps, 1))[:n]
    got = eng.scalar_inv(big)
    assert bad_rows(got, big_want).size == 0, bad_rows(got, big_want)[:8]
    out = dev_empty((n, 4), torch.int64)
    eng.scalar_inv_dev(to_dev(big), out, n)
    eng.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), big_want)
    with pytest.raises(FourQError):
        eng.scalar_inv_dev(to_dev(big).data_ptr() + 8, out, 4)


@pytest.mark.parametrize("k", SHIPPED_K)
def test_scalar_inv_zeros_never_touch_their_neighbours(eng, k):
    """With K forced: the same output as every other K; zeros at 5 % random positions; an all-zero batch; and exactly one zero in every
    lane's K-group, at each slot j in turn (lane t owns t, t + T, ..., T = ceil(n / K))."""
    _, words, want = inversion_inputs()
    rng = np.random.default_rng(5)
    with fresh_engine(eng, k) as e:
        assert bad_rows(e.scalar_inv(words), want).size == 0
        with pytest.raises(FourQError):
            e.set_scinv_group(4)                                    # not a shipped K
        assert bad_rows(e.prim("SC_INV", words[:65]), want[:65]).size == 0
        units = np.flatnonzero(want.any(axis=1))
        n = 1003                                                    # T = 1003, 126 or 63: the last lanes' groups run past the end for K > 1
        base, base_want = words[units[:n]].copy(), want[units[:n]].copy()
        hit = rng.random(n) < 0.05
        x, w = base.copy(), base_want.copy()
        x[hit], w[hit] = 0, 0
        x[np.flatnonzero(hit)[::3]] = codec.pack_scalars([N])[0]   # every third of them N itself, and after those 2N: zero modulo N, not in the words
        x[np.flatnonzero(hit)[1::3]] = codec.pack_scalars([2 * N])[0]
        assert 30 <= hit.sum() <= 80
        got = e.scalar_inv(x)
        assert bad_rows(got, w).size == 0, ("random zeros", bad_rows(got, w)[:8])
        assert not e.scalar_inv(np.zeros((n, 4), dtype=np.uint64)).any()
        T = -(-n // k)
        for j in range(k):
            x, w = base.copy(), base_want.copy()
            ids = np.arange(T) + j * T
            ids = ids[ids < n]
            x[ids], w[ids] = 0, 0
            got = e.scalar_inv(x)
            assert bad_rows(got, w).size == 0, ("slot", j, bad_rows(got, w)[:8])


# ---- 2. blind -----------------------------------------------------------------------------------------------------------------------------
def test_blind_batch_sizes_and_strides(eng):
    c = batch()
    for n in SIZES:
        for m in (c["m160"], c["m163"]):
            got, st = eng.oprf_blind(m[:n], c["r"][:n], c["lens"][:n], dst=DST)
            assert got.shape == (n, 32) and not st.any(), (n, m.shape[1])
            assert bad_rows(got, c["blinded"][:n]).size == 0, (n, m.shape[1], bad_rows(got, c["blinded"][:n])[:8])
    assert eng.oprf_blind(np.zeros((0, 16), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint64), dst=DST)[0].shape == (0, 32)


def test_blind_zero_blinds_and_non_canonical_blinds(eng):
    c = batch()
    n = 65
    r = list(c["blinds"][:n])
    for i, z in zip((0, 7, 64), (0, N, 2 * N)):
        r[i] = z
    for i in (1, 2, 3):                                             # r + N is the same blind
        r[i] = c["blinds"][i] % N + N
    got, st = eng.oprf_blind(c["m160"][:n], codec.pack_scalars(r), c["lens"][:n], dst=DST)
    want, wst = c["blinded"][:n].copy(), np.zeros(n, dtype=np.uint8)
    want[[0, 7, 64]], wst[[0, 7, 64]] = 0, _lib.OPRF_BLIND_ZERO
    assert np.array_equal(st, wst) and bad_rows(got, want).size == 0


# ---- 3. evaluate --------------------------------------------------------------------------------------------------------------------------
def test_evaluate_against_the_oracle_and_dh_bytes_on_adversarial_strings(eng):
    import adversarial_points as adv
    c = batch()
    got, st = eng.oprf_evaluate(c["k"], c["blinded"])
    assert not st.any() and bad_rows(got, c["evaluated"]).size == 0
    raw = rows_of([b for _, _, b in adv.all_strings()], 32)
    mixed = np.empty((2 * len(raw), 32), dtype=np.uint8)
    mixed[0::2], mixed[1::2] = raw, c["blinded"][np.arange(len(raw)) % 257]
    want, wst = eng.dh_bytes(np.tile(c["k"], (len(mixed), 1)), mixed)
    got, st = eng.oprf_evaluate(c["k"], mixed)
    assert np.array_equal(st, wst) and np.array_equal(got, want)
    assert len(set(wst.tolist())) >= 4 and not got[wst != 0].any()
    zero_key, st = eng.oprf_evaluate(codec.pack_scalars([N])[0], c["blinded"][:9])
    assert (st == _lib.DH_NEUTRAL).all() and not zero_key.any()


# ---- 4. finalize and eval -----------------------------------------------------------------------------------------------------------------
def test_fixture_rows_and_the_bytes_module(eng, golden):
    cases = golden("oprf.json", raw=True)["rows"]
    for dst_hex in sorted({c["dst"] for c in cases}):
        sel = [c for c in cases if c["dst"] == dst_hex]
        dst = bytes.fromhex(dst_hex)
        m, lens = codec.pack_messages([bytes.fromhex(c["msg"]) for c in sel])
        r = codec.pack_scalars([int(c["r"], 16) for c in sel])
        blinded, st = eng.oprf_blind(m, r, lens, dst=dst)
        assert not st.any() and [x.tobytes().hex() for x in blinded] == [c["blinded"] for c in sel]
        out, st = eng.oprf_finalize(m, r, rows_of([bytes.fromhex(c["evaluated"]) for c in sel], 32), lens, dst=dst)
        assert not st.any() and [x.tobytes().hex() for x in out] == [c["output"] for c in sel]
        for i, c in enumerate(sel):                                 # every row has a key of its own
            k = codec.pack_scalars([int(c["key"], 16)])[0]
            ev, st = eng.oprf_evaluate(k, blinded[i:i + 1])
            assert not st.any() and ev[0].tobytes().hex() == c["evaluated"]
            out, st = eng.oprf_eval(k, m[i:i + 1], lens[i:i + 1], dst=dst)
            assert not st.any() and out[0].tobytes().hex() == c["output"]
    if not eng.ct_select:                                           # the bytes module runs on the process-wide engine: once is enough
        from fourq_amd import oprf
        r, blinded = oprf.blind(oprf.KAT_MSG, oprf.KAT_DST, oprf.KAT_BLIND)
        assert (r, blinded.hex()) == (oprf.KAT_BLIND, oprf.KAT_BLINDED)
        evaluated = oprf.evaluate(oprf.KAT_KEY, blinded)
        assert evaluated.hex() == oprf.KAT_EVALUATED
        assert oprf.finalize(oprf.KAT_MSG, oprf.KAT_DST, r, evaluated).hex() == oprf.KAT_OUTPUT == oprf.evaluate_direct(oprf.KAT_KEY, oprf.KAT_MSG, oprf.KAT_DST).hex()
        r2, blinded2 = oprf.blind(oprf.KAT_MSG, oprf.KAT_DST)      # a fresh blind: another element, the same output
        assert 1 <= r2 < N and blinded2 != blinded
        assert oprf.finalize(oprf.KAT_MSG, oprf.KAT_DST, r2, oprf.evaluate(oprf.KAT_KEY, blinded2)).hex() == oprf.KAT_OUTPUT
        with pytest.raises(ValueError):
            oprf.blind(b"x", b"dst", N)


def test_protocol_round_trip_equals_eval_equals_the_restatement(eng):
    c = batch()
    for m in (c["m160"], c["m163"]):
        blinded, st = eng.oprf_blind(m, c["r"], c["lens"], dst=DST)
        evaluated, st2 = eng.oprf_evaluate(c["k"], blinded)
        out, st3 = eng.oprf_finalize(m, c["r"], evaluated, c["lens"], dst=DST)
        direct, st4 = eng.oprf_eval(c["k"], m, c["lens"], dst=DST)
        assert not (st.any() or st2.any() or st3.any() or st4.any())
        assert bad_rows(out, c["output"]).size == 0 and bad_rows(direct, c["output"]).size == 0, m.shape[1]
    for n in SIZES[:-1]:
        out, _ = eng.oprf_finalize(c["m160"][:n], c["r"][:n], c["evaluated"][:n], c["lens"][:n], dst=DST)
        direct, _ = eng.oprf_eval(c["k"], c["m163"][:n], c["lens"][:n], dst=DST)
        assert bad_rows(out, c["output"][:n]).size == 0 and bad_rows(direct, c["output"][:n]).size == 0, n
    other, _ = eng.oprf_eval(c["k"], c["m160"][:9], c["lens"][:9], dst=DST + b"!")
    assert bad_rows(other, c["output"][:9]).size == 9              # dst separates
    zero_key, st = eng.oprf_eval(codec.pack_scalars([2 * N])[0], c["m160"][:9], c["lens"][:9], dst=DST)
    assert (st == _lib.DH_NEUTRAL).all() and not zero_key.any()


def test_finalize_status_precedence(eng):
    """an element that does not decode: 16 + code and 64 zero bytes, also where the blind is zero; a zero blind alone: BLIND_ZERO; the
    neighbours are exact"""
    c = batch()
    n = 65
    z, r = c["evaluated"][:n].copy(), list(c["blinds"][:n])
    neutral = bytes([1] + [0] * 31)                                 # DECODE_REF_ATTRIBUTE_ERROR
    reserved = bytes(15) + b"\x80" + bytes(16)                      # DECODE_RESERVED_BIT
    z[3], z[4], z[64] = list(neutral), list(reserved), list(neutral)
    r[4], r[9], r[10] = 0, N, 0
    want, wst = c["output"][:n].copy(), np.zeros(n, dtype=np.uint8)
    wst[[3, 64]], wst[4], wst[[9, 10]] = 16 + _lib.DECODE_REF_ATTRIBUTE_ERROR, 16 + _lib.DECODE_RESERVED_BIT, _lib.OPRF_BLIND_ZERO
    want[wst != 0] = 0
    for k_rows in (n, 9):                                           # with and without neighbours in other waves
        got, st = eng.oprf_finalize(c["m160"][:k_rows], codec.pack_scalars(r[:k_rows]), z[:k_rows], c["lens"][:k_rows], dst=DST)
        assert np.array_equal(st, wst[:k_rows]) and bad_rows(got, want[:k_rows]).size == 0


# ---- 5. one large shape per call, against the composition of calls other tests pin --------------------------------------------------------
def test_large_shapes_against_the_composition(eng):
    n = eng.lanes + 257                                             # the fused route plus a tail; several elements per inversion
    rng = np.random.default_rng(77)
    m = rng.integers(0, 256, size=(n, 48), dtype=np.uint8)
    lens = rng.integers(0, 49, size=n, dtype=np.uint32)
    r = rng.integers(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    r[5], r[n - 1] = 0, codec.pack_scalars([N])[0]
    zero = np.zeros(n, dtype=bool)
    zero[[5, n - 1]] = True
    k = codec.pack_scalars([0x1234567890ABCDEF << 128 | 0xFEDCBA])[0]
    # blind = hash_to_curve(affine) -> mul_affine -> encode
    want = eng.encode(eng.mul_affine(r, eng.hash_to_curve(m, lens, dst=DST, affine=True)))
    want[zero] = 0
    blinded, st = eng.oprf_blind(m, r, lens, dst=DST)
    assert np.array_equal(st, np.where(zero, _lib.OPRF_BLIND_ZERO, 0)) and bad_rows(blinded, want).size == 0
    # evaluate = dh_bytes with the key tiled (the zeroed rows do not decode: the same status on both sides)
    want, wst = eng.dh_bytes(np.tile(k, (n, 1)), blinded)
    evaluated, st = eng.oprf_evaluate(k, blinded)
    assert np.array_equal(st, wst) and np.array_equal(evaluated, want) and (wst[zero] != 0).all() and not wst[~zero].any()
    # finalize = mul_bytes with host-side inverses -> sha512 over host-built strings
    inv = inv_words(codec.unpack_scalars(r))
    e32, est = eng.mul_bytes(inv, evaluated)
    tail = b"Finalize" + DST + bytes([len(DST)])
    strings = np.zeros((n, 32 + 48 + len(tail)), dtype=np.uint8)
    strings[:, :32] = e32
    for ln in range(49):                                            # msg and tail behind E, row by row of one length
        sel = np.flatnonzero(lens == ln)
        strings[sel[:, None], 32 + np.arange(ln)[None, :]] = m[sel, :ln]
        strings[sel[:, None], 32 + ln + np.arange(len(tail))[None, :]] = np.frombuffer(tail, dtype=np.uint8)
    want = eng.sha512(strings, (32 + lens + len(tail)).astype(np.uint32))
    wst = np.where(est != 0, est, np.where(zero, _lib.OPRF_BLIND_ZERO, 0)).astype(np.uint8)     # decode first, then the zero blind
    want[wst != 0] = 0
    out, st = eng.oprf_finalize(m, r, evaluated, lens, dst=DST)
    assert np.array_equal(st, wst) and (wst[zero] != 0).all() and not wst[~zero].any() and bad_rows(out, want).size == 0, bad_rows(out, want)[:8]
    # eval agrees with the round trip on every good row
    direct, st = eng.oprf_eval(k, m, lens, dst=DST)
    assert not st.any() and bad_rows(direct[~zero], out[~zero]).size == 0


def test_host_calls_over_several_chunks_equal_the_dev_forms(eng):
    """blind, finalize and eval cut into chunks of `lanes` rows (the message matrix and the lengths are two of a chunk's arrays) against the
    _dev forms on the same bytes, which the other tests pin against the restatement at small n."""
    import torch
    n, stride = 2 * eng.lanes + 77, 40
    rng = np.random.default_rng(79)
    m = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    lens = rng.integers(0, stride + 1, size=n, dtype=np.uint32)
    r = rng.integers(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    r[7] = 0
    k = codec.pack_scalars([0x1234567890ABCDEF << 128 | 0xFEDCBA])[0]
    d_m, d_lens, d_r = to_dev(m), to_dev(lens), to_dev(r)
    out32, out64, st = dev_empty((n, 32), torch.uint8), dev_empty((n, 64), torch.uint8), dev_empty(n, torch.uint8)

    blinded, bst = eng.oprf_blind(m, r, lens, dst=DST)
    assert eng.host_stats()["chunks"] > 1
    eng.oprf_blind_dev(d_m, stride, d_lens, 0, d_r, out32, st, n, dst=DST)
    eng.sync()
    assert np.array_equal(blinded, out32.cpu().numpy()) and np.array_equal(bst, st.cpu().numpy()) and bst[7] == _lib.OPRF_BLIND_ZERO and bst.sum() == bst[7]

    final, fst = eng.oprf_finalize(m, r, blinded, lens, dst=DST)     # row 7 is all zero: it does not decode
    assert eng.host_stats()["chunks"] > 1
    eng.oprf_finalize_dev(d_m, stride, d_lens, 0, d_r, out32, out64, st, n, dst=DST)
    eng.sync()
    assert np.array_equal(final, out64.cpu().numpy()) and np.array_equal(fst, st.cpu().numpy()) and np.flatnonzero(fst).tolist() == [7]

    direct, dst_ = eng.oprf_eval(k, m, lens, dst=DST)
    assert eng.host_stats()["chunks"] > 1
    eng.oprf_eval_dev(k, d_m, stride, d_lens, 0, out64, st, n, dst=DST)
    eng.sync()
    assert np.array_equal(direct, out64.cpu().numpy()) and np.array_equal(dst_, st.cpu().numpy()) and not dst_.any()


# ---- 6. the _dev forms --------------------------------------------------------------------------------------------------------------------
def test_dev_forms_clamp_and_refuse_misaligned_pointers(eng):
    import torch
    c = batch()
    n, stride = 130, 40
    m = np.ascontiguousarray(c["m160"][:n, :stride])
    lens = np.minimum(c["lens"][:n], stride).astype(np.uint32)
    over = lens.copy()
    over[::3] = stride + 9
    clamped = np.where(over > stride, _lib.SIG_MSG_CLAMPED, 0).astype(np.uint8)
    msgs = [m[i, :min(int(over[i]), stride)].tobytes() for i in range(n)]
    d_m, d_len, d_r = to_dev(m), to_dev(over), to_dev(c["r"][:n])
    out32, out64, st = dev_empty((n, 32), torch.uint8), dev_empty((n, 64), torch.uint8), dev_empty(n, torch.uint8)
    eng.oprf_blind_dev(d_m, stride, d_len, 0, d_r, out32, st, n, dst=DST)
    eng.sync()
    want = rows_of([ref.blind(msgs[i], DST, c["blinds"][i])[0] for i in range(n)], 32)
    want[clamped != 0] = 0
    assert np.array_equal(st.cpu().numpy(), clamped) and bad_rows(out32.cpu().numpy(), want).size == 0
    # evaluate, then finalize and eval on the clamped rows' honest lengths: the round trip on the device
    d_lens = to_dev(lens)
    eng.oprf_blind_dev(d_m, stride, d_lens, 0, d_r, out32, st, n, dst=DST)
    ev = dev_empty((n, 32), torch.uint8)
    eng.oprf_evaluate_dev(c["k"], out32, ev, st, n)
    eng.oprf_finalize_dev(d_m, stride, d_len, 0, d_r, ev, out64, st, n, dst=DST)
    eng.sync()
    want = rows_of([ref.evaluate_direct(c["key"], m[i, :lens[i]].tobytes(), DST)[0] for i in range(n)], 64)
    want_clamped = want.copy()
    want_clamped[clamped != 0] = 0
    assert np.array_equal(st.cpu().numpy(), clamped) and bad_rows(out64.cpu().numpy(), want_clamped).size == 0
    eng.oprf_eval_dev(c["k"], d_m, stride, d_len, 0, out64, st, n, dst=DST)
    eng.sync()
    assert np.array_equal(st.cpu().numpy(), clamped) and bad_rows(out64.cpu().numpy(), want_clamped).size == 0
    eng.oprf_eval_dev(c["k"], d_m, stride, None, stride, out64, st, n, dst=DST)            # lens = NULL: every row whole
    eng.sync()
    whole = rows_of([ref.evaluate_direct(c["key"], m[i].tobytes(), DST)[0] for i in range(16)], 64)
    assert not st.cpu().numpy().any() and bad_rows(out64.cpu().numpy()[:16], whole).size == 0
    for call in (lambda: eng.oprf_blind_dev(d_m, stride, d_len, 0, d_r.data_ptr() + 8, out32, st, 4, dst=DST),
                 lambda: eng.oprf_blind_dev(d_m.data_ptr() + 8, stride, d_len, 0, d_r, out32, st, 4, dst=DST),
                 lambda: eng.oprf_evaluate_dev(c["k"], out32.data_ptr() + 8, ev, st, 4),
                 lambda: eng.oprf_finalize_dev(d_m, stride, d_len, 0, d_r, ev.data_ptr() + 8, out64, st, 4, dst=DST),
                 lambda: eng.oprf_eval_dev(c["k"], d_m, stride, d_len, 0, out64.data_ptr() + 8, st, 4, dst=DST),
                 lambda: eng.oprf_eval_dev(c["k"], d_m, stride, d_len, 0, out64, st, 4, dst=b"")):
        with pytest.raises(FourQError):
            call()
    with pytest.raises(FourQError):
        eng.oprf_blind(m, c["r"][:n], over, dst=DST)                # the host form looks at the lengths


def test_finalize_dev_can_be_captured_into_a_hip_graph(eng):
    import torch
    dev = torch.device("cuda", 0)
    c = batch()
    n = 128
    m, lens = c["m160"], c["lens"]
    d_m, d_len, d_r, d_z = to_dev(m[:n]), to_dev(lens[:n]), to_dev(c["r"][:n]), to_dev(c["evaluated"][:n])
    out, st = torch.zeros((n, 64), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    try:
        eng.reserve(n)
        eng.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            eng.oprf_finalize_dev(d_m, m.shape[1], d_len, 0, d_r, d_z, out, st, n, dst=DST)
            graph.capture_end()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert bad_rows(out.cpu().numpy(), c["output"][:n]).size == 0 and not st.cpu().numpy().any()
        for d, a in ((d_m, m), (d_len, lens), (d_r, c["r"]), (d_z, c["evaluated"])):            # new rows in the captured buffers
            d.copy_(to_dev(a[n:2 * n]))
        graph.replay()
        torch.cuda.synchronize()
        assert bad_rows(out.cpu().numpy(), c["output"][n:2 * n]).size == 0 and not st.cpu().numpy().any()
    finally:
        eng.set_stream(None)


# ---- 7. several devices -------------------------------------------------------------------------------------------------------------------
def test_multi_engine(eng):
    from fourq_amd import MultiEngine, device_count
    c = batch()
    count = device_count()
    with MultiEngine(list(range(count)) if count > 1 else [0, 0]) as multi:
        multi.ct_select = eng.ct_select
        blinded, st = multi.oprf_blind(c["m163"], c["r"], c["lens"], dst=DST)
        assert not st.any() and np.array_equal(blinded, c["blinded"])
        evaluated, st = multi.oprf_evaluate(c["k"], blinded)
        assert not st.any() and np.array_equal(evaluated, c["evaluated"])
        out, st = multi.oprf_finalize(c["m163"], c["r"], evaluated, c["lens"], dst=DST)
        assert not st.any() and np.array_equal(out, c["output"])
        out, st = multi.oprf_eval(c["k"], c["m160"], c["lens"], dst=DST)
        assert not st.any() and np.array_equal(out, c["output"])


# ---- 8. the C ABI from C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_c_host_program(eng, tmp_path):
    from fourq_amd.build import LIB_PATH
    src = os.path.join(ROOT, "tests", "c", "oprf_check.c")
    exe, libdir = str(tmp_path / "oprf_check"), os.path.dirname(LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                    "-L", libdir, "-lfourq_amd", "-Wl,-rpath," + libdir], check=True)
    c = batch()
    n, m = 257, c["m163"]
    path = tmp_path / "vectors.bin"
    with open(path, "wb") as fh:
        for v in (n, 1 if eng.ct_select else 0, m.shape[1], len(DST)):
            fh.write(np.uint64(v).tobytes())
        fh.write(DST + bytes(256 - len(DST)))
        fh.write(m.tobytes())
        fh.write(c["lens"].astype("<u4").tobytes())
        fh.write(c["r"].astype("<u8").tobytes())
        fh.write(c["k"].astype("<u8").tobytes())
        fh.write(inv_words(c["blinds"]).astype("<u8").tobytes())
        fh.write(c["blinded"].tobytes())
        fh.write(c["evaluated"].tobytes())
        fh.write(c["output"].tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")     # no PyTorch in a C program: the system HIP runtime
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "rows bit-exact through the C ABI" in proc.stdout
