"""Signatures of registered keys on the device (fourq_keyset_*, fourq_keyset_sig_verify*): the key set's statuses, the keyed verify and the
keyed double multiplication against the fixture made with the reference's point functions (tests/golden/keyset.json), against the unkeyed
calls on keys[ids] byte for byte, and against the restatement's signatures (tests/sig_ref.py) at scale.  Every test takes `eng`: table
selection by address (the two combs in one accumulator) and constant-time selection (the existing routes on the gathered key bytes)."""
import ctypes
import random

import numpy as np
import pytest

import curve4q_oracle as o
import keyset_ref as kref
import sig_ref as ref
from fourq_amd import _lib, codec
from test_gpu_sig import bad_rows, byte_rows, g_comb, to_dev
from test_keyset_oracle import fixture
from test_sig_oracle import off_curve_key

pytestmark = pytest.mark.gpu

POOL = 256                                  # secret keys every test draws its key sets from
ROW_TAMPERS = ["msg bit", "R bit", "s bit", "s + N", "length one short"]
NOT_ON_CURVE = ref.BYTES_DECODE_BASE + ref.DECODE_NOT_ON_CURVE
_cache = {}


def pool():
    """(sks, pks) of POOL honest keys, the restatement's; per session"""
    if "pool" not in _cache:
        raw = np.random.default_rng(7100).integers(0, 256, size=(POOL, 32), dtype=np.uint8)
        sks = [r.tobytes() for r in raw]
        _cache["pool"] = (sks, ref.batch_keygen(sks))
    return _cache["pool"]


def signed_rows(n, key_of_row, seed):
    """n messages of mixed lengths and the restatement's signatures under pool key key_of_row[i]: (msgs, sigs)"""
    sks, pks = pool()
    rng = random.Random(seed)
    blob = np.random.default_rng(seed).integers(0, 256, size=1 << 12, dtype=np.uint8).tobytes()
    lengths = [0, 1, 15, 16, 17, 47, 48, 79, 80, 111, 112, 127, 128, 129, 200]
    msgs = []
    for i in range(n):
        ln = lengths[i % len(lengths)] if i % 3 else rng.randrange(2, 240)
        at = rng.randrange(len(blob) - 256)
        msgs.append(blob[at:at + ln])
    sigs = ref.batch_sign([sks[j] for j in key_of_row], [pks[j] for j in key_of_row], msgs)
    return msgs, sigs


def spoil(msgs, sigs, every, offset=0):
    """every `every`-th row spoiled by the row-level tamper classes in turn; returns the rows touched"""
    touched = []
    for j, i in enumerate(range(offset, len(msgs), every)):
        how = ROW_TAMPERS[j % len(ROW_TAMPERS)]
        if how in ("msg bit", "length one short") and len(msgs[i]) < 2:
            how = "R bit"
        if how == "msg bit":
            m = bytearray(msgs[i]); m[len(m) // 2] ^= 4; msgs[i] = bytes(m)
        elif how == "length one short":
            msgs[i] = msgs[i][:-1]
        elif how == "R bit":
            sigs[i, 7] ^= 1
        elif how == "s bit":
            sigs[i, 32 + 3] ^= 8
        else:
            sigs[i, 32:] = np.frombuffer((ref.LE(sigs[i, 32:].tobytes()) + o.N).to_bytes(32, "little"), dtype=np.uint8)
        touched.append(i)
    return touched


def dev_verify_keyed(eng, ids, matrix, lens, sigs):
    import torch
    dev = torch.device("cuda", 0)
    n = len(ids)
    ok, st = torch.full((n,), 7, dtype=torch.uint8, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
    eng.sig_verify_keyed_dev(to_dev(np.asarray(ids, dtype=np.uint32)), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, to_dev(sigs), ok, st, n)
    eng.sync()
    return ok.cpu().numpy(), st.cpu().numpy()


def dev_double_mul_keyed(eng, k, l, ids):
    import torch
    dev = torch.device("cuda", 0)
    n = len(ids)
    out, st = torch.full((n, 32), 7, dtype=torch.uint8, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
    eng.keyset_double_mul_bytes_dev(to_dev(k.view(np.int64)), to_dev(l.view(np.int64)), to_dev(np.asarray(ids, dtype=np.uint32)), out, st, n)
    eng.sync()
    return out.cpu().numpy(), st.cpu().numpy()


# ---- 1. rows computed with the real reference's point functions ------------------------------------------------------------------
def test_fixture_exact(eng):
    keys, statuses, rows, scalar_rows = fixture()
    g_comb(eng)
    got = eng.keyset_set(byte_rows(keys, 32))
    assert got.dtype == np.uint8 and list(got) == statuses and eng.keyset_count() == len(keys)
    ids = np.array([r[1] for r in rows], dtype=np.uint32)
    matrix, lens = codec.pack_messages([r[2] for r in rows])
    sigs = byte_rows([r[3] for r in rows], 64)
    want_ok, want_st = np.array([r[4] for r in rows], dtype=np.uint8), np.array([r[5] for r in rows], dtype=np.uint8)
    ok, st = eng.sig_verify_keyed(ids, matrix, sigs, lens)
    assert np.array_equal(ok, want_ok), [rows[i][0] for i in np.flatnonzero(ok != want_ok)]
    assert np.array_equal(st, want_st), [rows[i][0] for i in np.flatnonzero(st != want_st)]
    ok, st = dev_verify_keyed(eng, ids, matrix, lens, sigs)
    assert np.array_equal(ok, want_ok) and np.array_equal(st, want_st)
    sid = np.array([r[0] for r in scalar_rows], dtype=np.uint32)
    k, l = codec.pack_scalars([r[1] for r in scalar_rows]), codec.pack_scalars([r[2] for r in scalar_rows])
    want_out, want_st = byte_rows([r[3] for r in scalar_rows], 32), np.array([r[4] for r in scalar_rows], dtype=np.uint8)
    out, st = eng.keyset_double_mul_bytes(k, l, sid)
    assert bad_rows(out, want_out).size == 0, [(scalar_rows[i][0], hex(scalar_rows[i][1]), hex(scalar_rows[i][2])) for i in bad_rows(out, want_out)]
    assert np.array_equal(st, want_st)
    out, st = dev_double_mul_keyed(eng, k, l, sid)
    assert bad_rows(out, want_out).size == 0 and np.array_equal(st, want_st)


# ---- 2. for an accepted key (and one that does not decode) the keyed calls are the unkeyed calls on keys[ids] ------------------------
def id_patterns(n, m, rng):
    return {"all equal": np.zeros(n, dtype=np.uint32), "the last key only": np.full(n, m - 1, dtype=np.uint32),
            "distinct in turn": (np.arange(n) % m).astype(np.uint32), "random": rng.integers(0, m, size=n).astype(np.uint32)}


@pytest.mark.parametrize("m", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_equivalence_with_the_unkeyed_calls(eng, golden, n, m):
    sks, pks = pool()
    comb = g_comb(eng)
    slots = list(range(m))                          # slot -> pool key; with three keys or more, slot 1 holds a key that does not decode
    keys = pks[:m].copy()
    if m >= 3:
        keys[1] = np.frombuffer(off_curve_key(golden), dtype=np.uint8)
    status = eng.keyset_set(keys)
    assert list(status) == [NOT_ON_CURVE if (m >= 3 and j == 1) else 0 for j in range(m)]
    rng = np.random.default_rng(1000 * n + m)
    edges = [0, 1, 2, o.N - 1, o.N, o.N + 1, (1 << 256) - 1]
    for name, ids in id_patterns(n, m, rng).items():
        msgs, sigs = signed_rows(n, [slots[i] for i in ids], 31 * n + m)
        spoil(msgs, sigs, 5, offset=2)
        matrix, lens = codec.pack_messages(msgs)
        want_ok, want_st = eng.sig_verify(keys[ids], matrix, sigs, lens, comb)
        ok, st = eng.sig_verify_keyed(ids, matrix, sigs, lens, comb)
        assert np.array_equal(ok, want_ok) and np.array_equal(st, want_st), name
        honest = np.array([not (m >= 3 and i == 1) for i in ids])
        assert ok[honest].sum() == honest.sum() - len([i for i in range(2, n, 5) if honest[i]]), name        # the others still verify
        scalars = [edges[int(v)] if v < len(edges) else int.from_bytes(rng.bytes(32), "little") for v in rng.integers(0, 3 * len(edges), size=2 * n)]
        k, l = codec.pack_scalars(scalars[:n]), codec.pack_scalars(scalars[n:])
        want_out, want_st = eng.double_mul_bytes(k, l, keys[ids], comb)
        out, st = eng.keyset_double_mul_bytes(k, l, ids, comb)
        assert bad_rows(out, want_out).size == 0 and np.array_equal(st, want_st), name
    if n == 64 and m == 64:
        assert sorted(id_patterns(n, m, rng)["distinct in turn"]) == list(range(64))


# ---- 3. one large batch over 256 keys against the restatement's signatures ----------------------------------------------------------
def test_verify_at_scale(eng):
    n = 1 << 16
    sks, pks = pool()
    g_comb(eng)
    assert not eng.keyset_set(pks).any()
    ids = np.random.default_rng(7300).integers(0, POOL, size=n).astype(np.uint32)
    if "scale" not in _cache:
        msgs, sigs = signed_rows(n, ids, 7301)
        touched = spoil(msgs, sigs, 97)
        _cache["scale"] = (codec.pack_messages(msgs), sigs, touched)
    (matrix, lens), sigs, touched = _cache["scale"]
    want = np.ones(n, dtype=np.uint8)
    want[touched] = 0
    ok, st = eng.sig_verify_keyed(ids, matrix, sigs, lens)
    assert np.array_equal(ok, want), np.flatnonzero(ok != want)[:8]
    assert set(np.unique(st)) == {0, ref.SIG_S_RANGE} and not st[want == 1].any()
    ok_d, st_d = dev_verify_keyed(eng, ids, matrix, lens, sigs)
    assert np.array_equal(ok_d, want) and np.array_equal(st_d, st)
    wrong = (ids + 1) % POOL                                        # every row under its neighbour's key: nothing verifies
    ok, st = dev_verify_keyed(eng, wrong, matrix, lens, sigs)
    assert not ok.any()


# ---- 4. statuses and their precedence ------------------------------------------------------------------------------------------------
def test_statuses_and_precedence(eng, golden):
    from fourq_amd import FourQError
    sks, pks = pool()
    fkeys, fstatuses, _, _ = fixture()
    g_comb(eng)
    slots = [0, None, 1, None, 2]                  # slot -> pool key; slot 1 does not decode, slot 3 is (-x, -y) of an honest key
    keys = np.stack([pks[0], np.frombuffer(off_curve_key(golden), dtype=np.uint8), pks[1], np.frombuffer(fkeys[4], dtype=np.uint8), pks[2]])
    assert list(eng.keyset_set(keys)) == [0, NOT_ON_CURVE, 0, _lib.KEYSET_NOT_ORDER_N, 0]
    n = 700
    ids = (np.arange(n) % 5).astype(np.uint32)
    msgs, sigs = signed_rows(n, [slots[i] if slots[i] is not None else 0 for i in ids], 7400)
    matrix, lens = codec.pack_messages(msgs)
    key_st = np.array([0, NOT_ON_CURVE, 0, _lib.KEYSET_NOT_ORDER_N, 0], dtype=np.uint8)
    want_st = key_st[ids]
    want_ok = (want_st == 0).astype(np.uint8)
    ok, st = eng.sig_verify_keyed(ids, matrix, sigs, lens)
    assert np.array_equal(ok, want_ok) and np.array_equal(st, want_st)                  # the refused keys' neighbours are untouched
    k = np.random.default_rng(7401).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    l = np.random.default_rng(7402).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    out, st = eng.keyset_double_mul_bytes(k, l, ids)
    want_out, _ = eng.double_mul_bytes(k, l, keys[ids])
    want_out[want_st != 0] = 0
    assert bad_rows(out, want_out).size == 0 and np.array_equal(st, want_st) and out[want_st == 0].any(axis=1).all()
    # an index outside the set: the host forms refuse the call, the _dev forms clamp it, report it and leave a zero row
    far = ids.copy()
    far[3::7] = 5
    far[4::7] = 0xFFFFFFFF
    for call in (lambda: eng.sig_verify_keyed(far, matrix, sigs, lens), lambda: eng.keyset_double_mul_bytes(k, l, far)):
        with pytest.raises(FourQError):
            call()
    outside = far >= 5
    st_far, ok_far = np.where(outside, _lib.KEYSET_ID_RANGE, want_st).astype(np.uint8), np.where(outside, 0, want_ok).astype(np.uint8)
    ok, st = dev_verify_keyed(eng, far, matrix, lens, sigs)
    assert np.array_equal(ok, ok_far) and np.array_equal(st, st_far)
    out, st = dev_double_mul_keyed(eng, k, l, far)
    want_far = want_out.copy()
    want_far[outside] = 0
    assert bad_rows(out, want_far).size == 0 and np.array_equal(st, st_far)
    # a clamped message comes before s >= N, the key's status before both, the index before everything
    big = sigs.copy()
    for i in range(0, n, 3):
        big[i, 32:] = np.frombuffer((ref.LE(sigs[i, 32:].tobytes()) + o.N).to_bytes(32, "little"), dtype=np.uint8)
    over = lens.copy()
    over[::2] = matrix.shape[1] + 1
    want = np.where(np.arange(n) % 3 == 0, ref.SIG_S_RANGE, 0)
    want = np.where(np.arange(n) % 2 == 0, _lib.SIG_MSG_CLAMPED, want)
    want = np.where(want_st != 0, want_st, want)
    want = np.where(outside, _lib.KEYSET_ID_RANGE, want).astype(np.uint8)
    ok, st = dev_verify_keyed(eng, far, matrix, over, big)
    assert np.array_equal(st, want) and np.array_equal(ok, (want == 0).astype(np.uint8))
    assert {0, ref.SIG_S_RANGE, _lib.SIG_MSG_CLAMPED, NOT_ON_CURVE, _lib.KEYSET_NOT_ORDER_N, _lib.KEYSET_ID_RANGE} == set(want)
    assert ((np.arange(n) % 6 == 0) & (want == _lib.SIG_MSG_CLAMPED)).any()              # a row that is both clamped and s >= N


# ---- 5. the set: none, replaced, a failed set, and what it must not touch -------------------------------------------------------------
def test_set_handling(eng):
    import torch
    from fourq_amd import Engine, FourQError
    sks, pks = pool()
    n = 300
    ids = (np.arange(n) % 4).astype(np.uint32)
    msgs, sigs = signed_rows(n, list(ids), 7500)                     # signed by pool keys 0..3
    matrix, lens = codec.pack_messages(msgs)
    k = np.random.default_rng(7501).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        comb = e.comb_table(codec.pack_point(ref.G1))
        e.comb_stage(comb)
        assert e.keyset_count() == 0
        for call in (lambda: e.sig_verify_keyed(ids, matrix, sigs, lens), lambda: e.keyset_double_mul_bytes(k, k, ids)):
            with pytest.raises(FourQError):                          # no set
                call()
        ok, st = e.sig_verify_keyed(ids[:0], matrix[:0], sigs[:0], lens[:0])
        assert ok.shape == (0,) and st.shape == (0,)                 # n == 0 touches nothing, set or no set
        # what the set must leave alone: the commitment bases and the staged comb
        e.commit_bases(e.commit_generators(3, b"keyset-test"))
        commit_before = e.commit_bytes(k[:30], 3)
        keygen_before = e.sig_keygen(pks[:50])
        assert not e.keyset_set(pks[:4]).any() and e.keyset_count() == 4
        assert np.array_equal(e.commit_bytes(k[:30], 3), commit_before) and np.array_equal(e.sig_keygen(pks[:50]), keygen_before)
        assert e.commit_bases_count == 3
        ok, st = e.sig_verify_keyed(ids, matrix, sigs, lens)
        assert ok.all() and not st.any()
        # replaced: the old indices now name the new keys
        assert not e.keyset_set(pks[[4, 1, 6, 7]]).any() and e.keyset_count() == 4
        ok, st = e.sig_verify_keyed(ids, matrix, sigs, lens)
        assert np.array_equal(ok, (ids == 1).astype(np.uint8)) and not st.any()
        # a failed set keeps the old one
        for bad in (np.zeros((0, 32), dtype=np.uint8), np.zeros((_lib.KEYSET_MAX_KEYS + 1, 32), dtype=np.uint8)):
            with pytest.raises(FourQError):
                e.keyset_set(bad)
        assert e.keyset_count() == 4
        ok2, st2 = e.sig_verify_keyed(ids, matrix, sigs, lens)
        assert np.array_equal(ok2, ok) and not st2.any()
        # the set survives a change of stream
        side = torch.cuda.Stream(device=torch.device("cuda", 0))
        e.set_stream(side.cuda_stream)
        try:
            ok3, _ = e.sig_verify_keyed(ids, matrix, sigs, lens)
        finally:
            e.set_stream(None)
        assert np.array_equal(ok3, ok) and e.keyset_count() == 4
        assert np.array_equal(e.commit_bytes(k[:30], 3), commit_before)


# ---- 6. reservation: unsynchronised _dev calls, and a graph ----------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [False, True])
def test_two_unsynchronised_dev_calls_on_one_context(eng, reserve):
    import torch
    from fourq_amd import Engine
    dev = torch.device("cuda", 0)
    sks, pks = pool()
    n1, n2 = 500, 3000                                               # the second call is larger than anything the context has seen
    ids = np.random.default_rng(7600).integers(0, 16, size=n2).astype(np.uint32)
    msgs, sigs = signed_rows(n2, list(ids), 7601)
    touched = spoil(msgs, sigs, 11)
    matrix, lens = codec.pack_messages(msgs)
    want = np.ones(n2, dtype=np.uint8)
    want[touched] = 0
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        e.comb_stage(e.comb_table(codec.pack_point(ref.G1)))
        e.keyset_set(pks[:16])
        if reserve:
            e.keyset_reserve(n2)
        d_ids, d_m, d_len, d_sig = to_dev(ids), to_dev(matrix), to_dev(lens), to_dev(sigs)
        ok1, st1 = torch.full((n1,), 7, dtype=torch.uint8, device=dev), torch.full((n1,), 7, dtype=torch.uint8, device=dev)
        ok2, st2 = torch.full((n2,), 7, dtype=torch.uint8, device=dev), torch.full((n2,), 7, dtype=torch.uint8, device=dev)
        e.sig_verify_keyed_dev(d_ids, d_m, matrix.shape[1], d_len, 0, d_sig, ok1, st1, n1)
        e.sig_verify_keyed_dev(d_ids, d_m, matrix.shape[1], d_len, 0, d_sig, ok2, st2, n2)
        e.sync()
        assert np.array_equal(ok1.cpu().numpy(), want[:n1]) and np.array_equal(ok2.cpu().numpy(), want)
        assert np.array_equal(st1.cpu().numpy(), st2.cpu().numpy()[:n1])


def test_keyed_verify_dev_can_be_captured_into_a_hip_graph(eng):
    import torch
    dev = torch.device("cuda", 0)
    sks, pks = pool()
    n = 3000
    ids = np.random.default_rng(7700).integers(0, 32, size=2 * n).astype(np.uint32)
    msgs, sigs = signed_rows(2 * n, list(ids), 7701)
    matrix, lens = codec.pack_messages(msgs)
    comb = g_comb(eng)
    eng.keyset_set(pks[:32])
    d_ids, d_m, d_len, d_sig = to_dev(ids[:n]), to_dev(matrix[:n]), to_dev(lens[:n]), to_dev(sigs[:n])
    ok, st = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    try:
        eng.keyset_reserve(n)
        eng.comb_stage(comb)                              # staged on this stream, outside the capture
        eng.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            eng.sig_verify_keyed_dev(d_ids, d_m, matrix.shape[1], d_len, 0, d_sig, ok, st, n)
            graph.capture_end()
        ok.zero_()
        st.fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        assert ok.cpu().numpy().all() and not st.cpu().numpy().any()
        spoiled = sigs[n:].copy()
        spoiled[::7, 50] ^= 0x20
        d_ids.copy_(to_dev(ids[n:])); d_m.copy_(to_dev(matrix[n:])); d_len.copy_(to_dev(lens[n:])); d_sig.copy_(to_dev(spoiled))
        graph.replay()
        torch.cuda.synchronize()
        want = np.ones(n, dtype=np.uint8)
        want[::7] = 0
        got_st = st.cpu().numpy()
        assert np.array_equal(ok.cpu().numpy(), want)
        assert set(np.unique(got_st)) <= {0, ref.SIG_S_RANGE} and not got_st[want == 1].any()
    finally:
        eng.set_stream(None)


# ---- 7. the chunked pipeline ----------------------------------------------------------------------------------------------------------
def test_host_calls_over_several_chunks_equal_the_dev_forms(eng):
    """One chunk is `lanes` rows.  Signed rows are tiled to 2 x lanes + 77 (the ids, messages and signatures of 4 096 rows repeat), a few
    spoiled."""
    sks, pks = pool()
    g_comb(eng)
    eng.keyset_set(pks[:64])
    base, n = 4096, 2 * eng.lanes + 77
    ids0 = np.random.default_rng(7800).integers(0, 64, size=base).astype(np.uint32)
    blob = np.random.default_rng(7801).integers(0, 256, size=(base, 24), dtype=np.uint8)
    msgs = [blob[i, :i % 25].tobytes() for i in range(base)]
    matrix0, lens0 = codec.pack_messages(msgs)
    sigs0 = ref.batch_sign([sks[j] for j in ids0], [pks[j] for j in ids0], msgs)
    reps = -(-n // base)
    ids, matrix, lens, sigs = np.tile(ids0, reps)[:n], np.tile(matrix0, (reps, 1))[:n], np.tile(lens0, reps)[:n], np.tile(sigs0, (reps, 1))[:n].copy()
    sigs[5::1001, 3] ^= 1
    want = np.ones(n, dtype=np.uint8)
    want[5::1001] = 0
    ok, st = eng.sig_verify_keyed(ids, matrix, sigs, lens)
    assert eng.host_stats()["chunks"] > 1
    d_ok, d_st = dev_verify_keyed(eng, ids, matrix, lens, sigs)
    assert np.array_equal(ok, d_ok) and np.array_equal(st, d_st) and np.array_equal(ok, want) and not st.any()
    k = np.random.default_rng(7802).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    l = np.random.default_rng(7803).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    out, st = eng.keyset_double_mul_bytes(k, l, ids)
    assert eng.host_stats()["chunks"] > 1
    d_out, d_st = dev_double_mul_keyed(eng, k, l, ids)
    assert np.array_equal(out, d_out) and np.array_equal(st, d_st) and not st.any()
    want_out, _ = eng.double_mul_bytes(k[:3000], l[:3000], pks[ids[:3000]])
    assert bad_rows(out[:3000], want_out).size == 0


# ---- 8. the argument contract ---------------------------------------------------------------------------------------------------------
def test_argument_contract(eng):
    import torch
    dev = torch.device("cuda", 0)
    sks, pks = pool()
    g_comb(eng)
    eng.keyset_set(pks[:4])
    lib, ctx = eng._lib, eng._ctx
    n = 64
    buf = lambda nbytes: torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    k, l, ids, out, st, ok, sig, msg = buf(32 * n), buf(32 * n), buf(4 * n), buf(32 * n), buf(n), buf(n), buf(64 * n), buf(16 * n)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    dm, vf = lib.fourq_keyset_double_mul_bytes_dev, lib.fourq_keyset_sig_verify_dev
    good_dm = [p(k), None, p(l), p(ids), p(out), p(st)]
    good_vf = [p(ids), None, p(msg), 16, None, 16, p(sig), p(ok), p(st)]
    assert dm(ctx, *good_dm, n) == _lib.OK and vf(ctx, *good_vf, n) == _lib.OK
    assert dm(None, *good_dm, n) == _lib.ERR_INVALID and vf(None, *good_vf, n) == _lib.ERR_INVALID
    for at in (0, 2, 3, 4, 5):                                       # every array of the double multiplication: NULL
        args = list(good_dm); args[at] = None
        assert dm(ctx, *args, n) == _lib.ERR_INVALID, at
    for at in (0, 6, 7, 8):
        args = list(good_vf); args[at] = None
        assert vf(ctx, *args, n) == _lib.ERR_INVALID, at
    for at, t in ((0, k), (2, l), (3, ids), (4, out)):               # misaligned: the scalars, the indices, the output rows
        args = list(good_dm); args[at] = p(t, 8)
        assert dm(ctx, *args, n) == _lib.ERR_INVALID, at
    for at, t in ((0, ids), (2, msg), (6, sig)):
        args = list(good_vf); args[at] = p(t, 4 if at == 0 else 8)
        assert vf(ctx, *args, n) == _lib.ERR_INVALID, at
    args = list(good_dm); args[5] = p(st, 1)                         # status and ok need not be aligned
    assert dm(ctx, *args, n) == _lib.OK
    args = list(good_vf); args[7] = p(ok, 1); args[8] = p(st, 3)
    assert vf(ctx, *args, n) == _lib.OK
    assert dm(ctx, *good_dm, _lib.MAX_BATCH + 1) == _lib.ERR_INVALID and vf(ctx, *good_vf, _lib.MAX_BATCH + 1) == _lib.ERR_INVALID
    eng.sync()
    out.fill_(9); st.fill_(9); ok.fill_(9)                           # n == 0: OK, nothing touched
    assert dm(ctx, *good_dm, 0) == _lib.OK and vf(ctx, *good_vf, 0) == _lib.OK
    eng.sync()
    assert (out.cpu().numpy() == 9).all() and (st.cpu().numpy() == 9).all() and (ok.cpu().numpy() == 9).all()
    assert lib.fourq_keyset_reserve(ctx, _lib.MAX_BATCH + 1) == _lib.ERR_INVALID
    assert lib.fourq_keyset_set(ctx, None, 1, None) == _lib.ERR_INVALID


# ---- 9. several devices ---------------------------------------------------------------------------------------------------------------
def test_multi_engine_with_one_device_equals_engine(eng, golden):
    from fourq_amd import MultiEngine
    sks, pks = pool()
    comb = g_comb(eng)
    keys = pks[:8].copy()
    keys[5] = np.frombuffer(off_curve_key(golden), dtype=np.uint8)
    n = 5000
    ids = np.random.default_rng(7900).integers(0, 8, size=n).astype(np.uint32)
    msgs, sigs = signed_rows(n, list(ids), 7901)
    spoil(msgs, sigs, 13)
    matrix, lens = codec.pack_messages(msgs)
    k = np.random.default_rng(7902).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    status = eng.keyset_set(keys)
    want = eng.sig_verify_keyed(ids, matrix, sigs, lens, comb) + eng.keyset_double_mul_bytes(k, k[::-1].copy(), ids, comb)
    with MultiEngine([0, 0]) as multi:
        multi.ct_select = eng.ct_select
        assert np.array_equal(multi.keyset_set(keys), status) and multi.keyset_count() == 8
        got = multi.sig_verify_keyed(ids, matrix, sigs, lens, comb) + multi.keyset_double_mul_bytes(k, k[::-1].copy(), ids, comb)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert 0 < want[0].sum() < n and set(np.unique(want[1])) == {0, ref.SIG_S_RANGE, NOT_ON_CURVE}
