"""Signatures from bytes on the device (fourq_sig_* / fourq_amd.schnorrq): keygen, sign and verify against the restatement in
tests/sig_ref.py -- hashlib, Python ints modulo N and the oracles' point functions; tests/test_sig_oracle.py pins it against rows the
real reference's point functions produced.  Every test takes `eng`: table selection by address and constant-time selection."""
import hashlib
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import curve4q_oracle as o
import sig_ref as ref
from conftest import ROOT
from fourq_amd import _lib, codec
from test_sig_oracle import TAMPERS, off_curve_key, rows, tampered

pytestmark = pytest.mark.gpu

G1_WORDS = codec.pack_point(ref.G1)
_cache = {}
BIG = (1 << 16) + 256          # the seeded batch every test draws from: one generation of lanes and a remainder


def g_comb(eng):
    if "comb" not in _cache:
        _cache["comb"] = eng.comb_table(G1_WORDS)
    eng.comb_stage(_cache["comb"])
    return _cache["comb"]


def byte_rows(items, width):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), width).copy()


def seeded_batch(n, seed):
    """sks, messages of mixed lengths (every block count of both hashed strings), and the restatement's pks and sigs; per session."""
    key = (n, seed)
    if key not in _cache:
        rng = random.Random(seed)
        raw = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
        sks = [r.tobytes() for r in raw]
        pool = np.random.default_rng(seed + 1).integers(0, 256, size=1 << 16, dtype=np.uint8).tobytes()
        lengths = [0, 1, 15, 16, 17, 47, 48, 79, 80, 111, 112, 127, 128, 129, 200]
        msgs = []
        for i in range(n):
            ln = lengths[i % len(lengths)] if i % 3 else rng.randrange(0, 240)
            at = rng.randrange(len(pool) - 256)
            msgs.append(pool[at:at + ln])
        pks = ref.batch_keygen(sks)
        sigs = ref.batch_sign(sks, pks, msgs)
        _cache[key] = (raw, msgs, pks, sigs)
    return _cache[key]


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(torch.device("cuda", 0))


def dev_verify(eng, pks, matrix, lens, sigs):
    import torch
    dev = torch.device("cuda", 0)
    n = len(pks)
    ok, st = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    eng.sig_verify_dev(to_dev(pks), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, to_dev(sigs), ok, st, n)
    eng.sync()
    return ok.cpu().numpy(), st.cpu().numpy()


def bad_rows(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))


# ---- 1. rows computed with the real reference's point functions ------------------------------------------------------------------
def test_golden_rows_exact_and_single_calls(eng, golden):
    cases = rows(golden)
    comb = g_comb(eng)
    sk, pk, sig = byte_rows([c["sk"] for c in cases], 32), byte_rows([c["pk"] for c in cases], 32), byte_rows([c["sig"] for c in cases], 64)
    matrix, lens = codec.pack_messages([c["msg"] for c in cases])
    assert matrix.shape[1] % 16 == 0 and matrix.shape[1] >= 1000 and list(lens) == [len(c["msg"]) for c in cases]
    got_pk = eng.sig_keygen(sk, comb)
    assert bad_rows(got_pk, pk).size == 0, [cases[i]["_label"] for i in bad_rows(got_pk, pk)]
    got_sig = eng.sig_sign(sk, pk, matrix, lens)
    assert bad_rows(got_sig, sig).size == 0, [cases[i]["_label"] for i in bad_rows(got_sig, sig)]
    ok, st = eng.sig_verify(pk, matrix, sig, lens)
    assert ok.all() and not st.any()
    # fourq_amd.schnorrq on bytes, through the process-wide engine in the same selection mode
    from fourq_amd import schnorrq
    from fourq_amd.engine import default_engine
    before = default_engine().ct_select
    default_engine().ct_select = eng.ct_select
    try:
        for c in cases[:3] + cases[-3:]:
            assert schnorrq.keygen(c["sk"]) == c["pk"]
            assert schnorrq.sign(c["sk"], c["msg"]) == c["sig"]
            assert schnorrq.verify(c["pk"], c["msg"], c["sig"]) is True
            assert schnorrq.verify(c["pk"], c["msg"] + b"x", c["sig"]) is False
        some = cases[5:25]
        assert schnorrq.sign_many([c["sk"] for c in some], [c["msg"] for c in some]) == [c["sig"] for c in some]
        assert schnorrq.verify_many([c["pk"] for c in some], [c["msg"] for c in some], [c["sig"] for c in some]) == [True] * len(some)
    finally:
        default_engine().ct_select = before


# ---- 2. at scale, host-pointer and device forms ----------------------------------------------------------------------------------
def test_keygen_sign_verify_at_scale(eng):
    import torch
    n = BIG
    sk, msgs, pks, sigs = seeded_batch(n, 6100)
    comb = g_comb(eng)
    matrix, lens = codec.pack_messages(msgs)
    got_pk = eng.sig_keygen(sk, comb)
    assert bad_rows(got_pk, pks).size == 0, bad_rows(got_pk, pks)[:8]
    got_sig = eng.sig_sign(sk, pks, matrix, lens)
    assert bad_rows(got_sig, sigs).size == 0, bad_rows(got_sig, sigs)[:8]
    ok, st = eng.sig_verify(pks, matrix, sigs, lens)
    assert ok.dtype == np.uint8 and np.array_equal(ok, np.ones(n, dtype=np.uint8)) and not st.any()
    # device-resident: one launch chain over the whole batch
    dev = torch.device("cuda", 0)
    d_sk, d_m, d_len = to_dev(sk), to_dev(matrix), to_dev(lens)
    d_pk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    d_sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    eng.sig_keygen_dev(d_sk, d_pk, n)
    eng.sig_sign_dev(d_sk, d_pk, d_m, matrix.shape[1], d_len, 0, d_sig, n)
    eng.sync()
    assert bad_rows(d_pk.cpu().numpy(), pks).size == 0 and bad_rows(d_sig.cpu().numpy(), sigs).size == 0
    ok, st = dev_verify(eng, pks, matrix, lens, sigs)
    assert ok.all() and not st.any()


def test_host_calls_over_several_chunks_equal_the_dev_forms(eng):
    """sign and verify cut into chunks (the message matrix and the lengths are two of a chunk's arrays) against the _dev forms on the same
    bytes, which the tests around this one pin against the restatement.  One chunk of sign is 4 x lanes rows, so it takes more than
    2 x lanes + 77 rows to make a second one; one of verify is `lanes` rows, and it runs on the first 2 x lanes + 77 of them."""
    import torch
    dev = torch.device("cuda", 0)
    n, nv, stride = 4 * eng.lanes + 77, 2 * eng.lanes + 77, 24
    g_comb(eng)
    rng = np.random.default_rng(6200)
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    matrix = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    lens = rng.integers(0, stride + 1, size=n, dtype=np.uint32)
    pk = eng.sig_keygen(sk)
    sig = eng.sig_sign(sk, pk, matrix, lens)
    assert eng.host_stats()["chunks"] > 1
    d_pk, d_m, d_len = to_dev(pk), to_dev(matrix), to_dev(lens)
    d_sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    eng.sig_sign_dev(to_dev(sk), d_pk, d_m, stride, d_len, 0, d_sig, n)
    eng.sync()
    assert np.array_equal(sig, d_sig.cpu().numpy())
    sig[5, 3] ^= 1                                                 # one row that does not verify, on both sides
    ok, st = eng.sig_verify(pk[:nv], matrix[:nv], sig[:nv], lens[:nv])
    assert eng.host_stats()["chunks"] > 1
    d_ok, d_st = dev_verify(eng, pk[:nv], matrix[:nv], lens[:nv], sig[:nv])
    assert np.array_equal(ok, d_ok) and np.array_equal(st, d_st) and ok.sum() == nv - 1 and not ok[5]


# ---- 3. the verifier must not say yes too often ----------------------------------------------------------------------------------
def test_every_tamper_class_inside_one_batch(eng, golden):
    n = 4096
    sk, msgs, pks, sigs = seeded_batch(BIG, 6100)
    g_comb(eng)
    refused = off_curve_key(golden)
    pk2, sig2, msgs2 = pks[:n].copy(), sigs[:n].copy(), list(msgs[:n])
    want_ok, want_st = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    seen = {how: 0 for how in TAMPERS}
    j = 0
    for i in range(0, n, 5):
        how = TAMPERS[j % len(TAMPERS)]
        j += 1
        if how in ("msg bit", "length one short") and len(msgs2[i]) < 2:
            how = "R bit"
        p, m, s = tampered(pk2[i].tobytes(), msgs2[i], sig2[i].tobytes(), how, refused)
        pk2[i], sig2[i], msgs2[i] = np.frombuffer(p, dtype=np.uint8), np.frombuffer(s, dtype=np.uint8), m
        want_ok[i], want_st[i] = ref.verify(p, m, s)                   # the restatement's verdict, row by row
        assert want_ok[i] == 0
        seen[how] += 1
    assert all(v >= 50 for v in seen.values()), seen
    assert {ref.SIG_S_RANGE, ref.BYTES_DECODE_BASE + ref.DECODE_RESERVED_BIT, ref.BYTES_DECODE_BASE + ref.DECODE_NOT_ON_CURVE} <= set(want_st)
    matrix, lens = codec.pack_messages(msgs2)
    ok, st = eng.sig_verify(pk2, matrix, sig2, lens)
    assert np.array_equal(ok, want_ok), np.flatnonzero(ok != want_ok)[:8]            # the untouched neighbours are still accepted
    assert np.array_equal(st, want_st), np.flatnonzero(st != want_st)[:8]
    ok_d, st_d = dev_verify(eng, pk2, matrix, lens, sig2)
    assert np.array_equal(ok_d, want_ok) and np.array_equal(st_d, want_st)
    # the _dev call clamps a length above the stride and says so; a key that does not decode still takes precedence
    over = lens.copy()
    over[1::5] = matrix.shape[1] + 1
    ok_d, st_d = dev_verify(eng, pk2, matrix, over, sig2)
    st_over = want_st.copy()
    st_over[1::5] = _lib.SIG_MSG_CLAMPED
    ok_over = want_ok.copy()
    ok_over[1::5] = 0
    assert np.array_equal(ok_d, ok_over) and np.array_equal(st_d, st_over)


# ---- 4. the byte-level call is the scalar-level call with the hash done on the device ----------------------------------------------
def test_equivalence_with_verify_bytes(eng, golden):
    n = 3000
    sk, msgs, pks, sigs = seeded_batch(BIG, 6100)
    comb = g_comb(eng)
    pk2, sig2, msgs2 = pks[:n].copy(), sigs[:n].copy(), list(msgs[:n])
    refused = off_curve_key(golden)
    for j, i in enumerate(range(0, n, 4)):
        how = [t for t in TAMPERS if t != "s + N"][j % (len(TAMPERS) - 1)]         # verify_bytes has no range check: s + N is left out here
        if how in ("msg bit", "length one short") and len(msgs2[i]) < 2:
            how = "s bit"
        p, m, s = tampered(pk2[i].tobytes(), msgs2[i], sig2[i].tobytes(), how, refused)
        if ref.LE(s[32:]) >= o.N:
            continue
        pk2[i], sig2[i], msgs2[i] = np.frombuffer(p, dtype=np.uint8), np.frombuffer(s, dtype=np.uint8), m
    h = codec.pack_scalars([ref.challenge(sig2[i, :32].tobytes(), pk2[i].tobytes(), msgs2[i]) for i in range(n)])
    s_words = np.ascontiguousarray(sig2[:, 32:]).view("<u8").reshape(n, 4)
    ok_b, st_b = eng.verify_bytes(s_words, h, pk2, np.ascontiguousarray(sig2[:, :32]), comb)
    matrix, lens = codec.pack_messages(msgs2)
    ok, st = eng.sig_verify(pk2, matrix, sig2, lens)
    assert np.array_equal(ok, ok_b) and np.array_equal(st, st_b)
    assert 0 < ok.sum() < n


# ---- 5. batch sizes ----------------------------------------------------------------------------------------------------------
def test_batch_sizes(eng):
    lanes = eng.lanes
    top = lanes + 1
    assert top <= BIG
    sk, msgs, pks, sigs = seeded_batch(BIG, 6100)
    g_comb(eng)
    matrix, lens = codec.pack_messages(msgs[:top])
    assert eng.sig_keygen(sk[:0]).shape == (0, 32) and eng.sig_sign(sk[:0], pks[:0], matrix[:0], lens[:0]).shape == (0, 64)
    ok, st = eng.sig_verify(pks[:0], matrix[:0], sigs[:0], lens[:0])
    assert ok.shape == (0,) and st.shape == (0,)
    for n in (1, 2, 255, 257, lanes // 4 - 3, lanes // 4, lanes + 1):
        assert bad_rows(eng.sig_keygen(sk[:n]), pks[:n]).size == 0, n
        assert bad_rows(eng.sig_sign(sk[:n], pks[:n], matrix[:n], lens[:n]), sigs[:n]).size == 0, n
        spoiled = sigs[:n].copy()
        spoiled[n // 2, 40] ^= 1
        ok, st = eng.sig_verify(pks[:n], matrix[:n], spoiled, lens[:n])
        assert ok.sum() == n - 1 and ok[n // 2] == 0 and not st.any(), n
        ok, st = dev_verify(eng, pks[:n], matrix[:n], lens[:n], sigs[:n])
        assert ok.all() and not st.any(), n
    # messages of one fixed length, lens = NULL; and empty messages through stride 0
    fixed = [m for m in msgs if len(m) == 48][:500]
    idx = [i for i, m in enumerate(msgs) if len(m) == 48][:500]
    m48 = byte_rows(fixed, 48)
    assert bad_rows(eng.sig_sign(sk[idx], pks[idx], m48), sigs[idx]).size == 0
    ok, st = eng.sig_verify(pks[idx], m48, sigs[idx])
    assert ok.all() and not st.any()
    idx0 = [i for i, m in enumerate(msgs) if len(m) == 0][:300]
    empty = np.zeros((len(idx0), 0), dtype=np.uint8)
    assert bad_rows(eng.sig_sign(sk[idx0], pks[idx0], empty), sigs[idx0]).size == 0
    ok, st = eng.sig_verify(pks[idx0], empty, sigs[idx0])
    assert ok.all() and not st.any()


# ---- 6. a reserved context only enqueues: sig_verify_dev in a graph ------------------------------------------------------------------
def test_sig_verify_dev_can_be_captured_into_a_hip_graph(eng):
    """Reserve, stage the comb, capture one sig_verify_dev, replay it on the captured inputs and once more on new ones (one capture,
    two replays)."""
    import torch
    dev = torch.device("cuda", 0)
    n = 3000
    sk, msgs, pks, sigs = seeded_batch(BIG, 6100)
    matrix, lens = codec.pack_messages(msgs[:2 * n])
    comb = g_comb(eng)
    d_pk, d_m, d_len, d_sig = to_dev(pks[:n]), to_dev(matrix[:n]), to_dev(lens[:n]), to_dev(sigs[:n])
    ok, st = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    try:
        eng.reserve(n)
        eng.comb_stage(comb)                              # staged on this stream, outside the capture
        eng.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            eng.sig_verify_dev(d_pk, d_m, matrix.shape[1], d_len, 0, d_sig, ok, st, n)
            graph.capture_end()
        ok.zero_()
        st.fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        assert ok.cpu().numpy().all() and not st.cpu().numpy().any()
        # new inputs in the captured buffers: the second half of the batch, every seventh signature spoiled
        spoiled = sigs[n:2 * n].copy()
        spoiled[::7, 50] ^= 0x20
        d_pk.copy_(to_dev(pks[n:2 * n])); d_m.copy_(to_dev(matrix[n:2 * n])); d_len.copy_(to_dev(lens[n:2 * n])); d_sig.copy_(to_dev(spoiled))
        graph.replay()
        torch.cuda.synchronize()
        want = np.ones(n, dtype=np.uint8)
        want[::7] = 0
        got_st = st.cpu().numpy()
        assert np.array_equal(ok.cpu().numpy(), want)
        assert set(np.unique(got_st)) <= {0, _lib.SIG_S_RANGE} and not got_st[want == 1].any()
    finally:
        eng.set_stream(None)


# ---- 7. several devices ------------------------------------------------------------------------------------------------------------
def test_multi_engine(eng):
    from fourq_amd import MultiEngine, device_count
    n = 40000
    sk, msgs, pks, sigs = seeded_batch(BIG, 6100)
    comb = g_comb(eng)
    matrix, lens = codec.pack_messages(msgs[:n])
    spoiled = sigs[:n].copy()
    spoiled[::13, 3] ^= 1
    want = np.ones(n, dtype=np.uint8)
    want[::13] = 0
    count = device_count()
    with MultiEngine(list(range(count)) if count > 1 else [0, 0]) as multi:
        multi.ct_select = eng.ct_select
        assert bad_rows(multi.sig_sign(sk[:n], pks[:n], matrix, lens, comb), sigs[:n]).size == 0
        ok, st = multi.sig_verify(pks[:n], matrix, spoiled, lens, comb)
        assert np.array_equal(ok, want) and not st.any()


# ---- 8. the C ABI from C -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_c_host_program_generates_signs_and_verifies(eng, golden, tmp_path):
    from fourq_amd.build import LIB_PATH
    cases = rows(golden)
    src = os.path.join(ROOT, "tests", "c", "sig_check.c")
    exe, libdir = str(tmp_path / "sig_check"), os.path.dirname(LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                    "-L", libdir, "-lfourq_amd", "-Wl,-rpath," + libdir], check=True)
    matrix, lens = codec.pack_messages([c["msg"] for c in cases])
    path = tmp_path / "vectors.bin"
    with open(path, "wb") as fh:
        for v in (len(cases), 1 if eng.ct_select else 0, matrix.shape[1]):
            fh.write(np.uint64(v).tobytes())
        fh.write(np.ascontiguousarray(G1_WORDS, dtype="<u8").tobytes())
        fh.write(byte_rows([c["sk"] for c in cases], 32).tobytes())
        fh.write(matrix.tobytes())
        fh.write(lens.astype("<u4").tobytes())
        fh.write(byte_rows([c["pk"] for c in cases], 32).tobytes())
        fh.write(byte_rows([c["sig"] for c in cases], 64).tobytes())
        fh.write(byte_rows([hashlib.sha512(c["msg"]).digest() for c in cases], 64).tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")     # no PyTorch in a C program: the system HIP runtime
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "signature rows bit-exact through the C ABI" in proc.stdout
