"""Hash to curve on the device (fourq_hash_to_field_* / fourq_map_to_curve_* / fourq_hash_to_curve_*, h2c.hip.h) against the CPU
restatement tests/h2c_ref.py: every message length across the block boundaries of all three hashed strings, every row alignment, the
map on its edge inputs and on non-canonical words, every batch-size class, both modes, both output forms, in both selection modes.
The restatement's answers are computed once per process and shared by both engines."""
import functools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import h2c_ref as ref
from fourq_amd import FourQError, _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ref.P
TAG = b"QUUX-V01-CS02-with-FourQ_XMD:SHA-512_ELL2_RO_"
DSTS = {1: b"D", 43: TAG[:43], 255: (TAG * 6)[:255]}
MODES = {"ro": ref.RO, "nu": ref.NU}
SIZES = (1, 63, 64, 65, 257, 4096)


def random_matrix(n, stride, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, stride), dtype=np.uint8)


def bad_rows(got, expect):
    got, expect = np.asarray(got).reshape(len(expect), -1), np.asarray(expect).reshape(len(expect), -1)
    return np.flatnonzero((got != expect).any(axis=1))


def words(rows):
    return np.array(rows, dtype=np.uint64).reshape(len(rows), -1)


@functools.lru_cache(maxsize=None)
def want_u(msg, dst, mode):
    return tuple(ref.hash_to_field(msg, dst, MODES[mode]))


@functools.lru_cache(maxsize=None)
def want_map(u):
    return ref.map_to_curve(u)


@functools.lru_cache(maxsize=None)
def want_affine(msg, dst, mode):
    Q = want_map(want_u(msg, dst, mode)[0])
    if mode == "ro":
        Q = ref.add_affine(Q, want_map(want_u(msg, dst, mode)[1]))
    x, y = ref.clear_cofactor(Q)
    return ref.canon(x), ref.canon(y)


def want_u_words(matrix, lens, dst, mode):
    return words([[w for u in want_u(matrix[i, :lens[i]].tobytes(), dst, mode) for w in ref.u_words(u)] for i in range(len(matrix))])


def want_affine_words(matrix, lens, dst, mode):
    return words([ref.affine_words(want_affine(matrix[i, :lens[i]].tobytes(), dst, mode)) for i in range(len(matrix))])


def want_bytes(matrix, lens, dst, mode):
    import curve4q_oracle as o
    rows = [bytes(o.encode(*want_affine(matrix[i, :lens[i]].tobytes(), dst, mode))) for i in range(len(matrix))]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """4 096 rows of mixed lengths (0 .. 150, every block count of b_0 for the 43-byte DST) in a 160-byte stride."""
    rng = random.Random(20261017)
    lens = np.array([rng.randrange(151) for _ in range(SIZES[-1])], dtype=np.uint32)
    lens[:8] = (0, 1, 63, 64, 65, 150, 16, 17)
    return random_matrix(SIZES[-1], 160, 11), lens


# ---- 1. hash_to_field ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_len", sorted(DSTS))
def test_hash_to_field_every_length_up_to_300(eng, dst_len):
    """Rows of 0 .. 300 bytes side by side, rows 16-byte aligned, 8-byte aligned and at odd addresses; the matrix is random, so every row
    has foreign bytes behind its length."""
    dst = DSTS[dst_len]
    lens = np.arange(301, dtype=np.uint32)
    for stride, mode in ((304, "ro"), (312, "ro"), (307, "ro"), (304, "nu")):
        m = random_matrix(301, stride, stride)
        got = eng.hash_to_field(m, lens, dst=dst, mode=mode)
        expect = want_u_words(m, lens, dst, mode)
        assert got.shape == (301, 2 if mode == "ro" else 1, 4)
        assert bad_rows(got, expect).size == 0, (stride, mode, bad_rows(got, expect)[:8])


def test_hash_to_field_ignores_what_lies_behind_a_row(eng):
    rng = random.Random(5)
    for stride in (160, 168, 163):
        lens = np.array([rng.randrange(stride + 1) for _ in range(512)], dtype=np.uint32)
        a, b = random_matrix(512, stride, 6), random_matrix(512, stride, 7)
        for i, ln in enumerate(lens):
            b[i, :ln] = a[i, :ln]                             # same messages, different bytes behind them
        ga, gb = eng.hash_to_field(a, lens, dst=DSTS[43]), eng.hash_to_field(b, lens, dst=DSTS[43])
        assert np.array_equal(ga, gb), stride
        assert bad_rows(ga[:64], want_u_words(a[:64], lens[:64], DSTS[43], "ro")).size == 0, stride


def test_hash_to_field_dev_fixed_length_and_clamping(eng):
    """lens = NULL with msg_len, on a matrix that starts 16 bytes into an allocation; a length above the stride is the clamped row's hash."""
    import torch
    dev = torch.device("cuda", 0)
    n = 130
    for stride in (37, 40, 48):
        m = random_matrix(n, stride, 2000 + stride)
        buf = torch.zeros(16 + n * stride, dtype=torch.uint8, device=dev)
        buf[16:] = torch.from_numpy(m.reshape(-1)).to(dev)
        out = torch.empty((n, 2, 4), dtype=torch.int64, device=dev)
        eng.hash_to_field_dev(buf.data_ptr() + 16, stride, None, stride - 5, out, n, dst=DSTS[43])
        eng.sync()
        assert bad_rows(out.cpu().numpy().view(np.uint64), want_u_words(m, np.full(n, stride - 5), DSTS[43], "ro")).size == 0, stride
        lens = np.array([random.Random(i).randrange(stride + 1) for i in range(n)], dtype=np.uint32)
        over = lens.copy()
        over[::3] = stride + 9
        eng.hash_to_field_dev(buf.data_ptr() + 16, stride, torch.from_numpy(over.view(np.int32)).to(dev), 0, out, n, dst=DSTS[43])
        eng.sync()
        assert bad_rows(out.cpu().numpy().view(np.uint64), want_u_words(m, np.minimum(over, stride), DSTS[43], "ro")).size == 0, stride
        out32 = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        eng.hash_to_curve_dev(buf.data_ptr() + 16, stride, torch.from_numpy(over.view(np.int32)).to(dev), 0, out32, n, dst=DSTS[43], mode="nu")
        eng.sync()
        assert bad_rows(out32.cpu().numpy(), want_bytes(m, np.minimum(over, stride), DSTS[43], "nu")).size == 0, stride
    # the same through the host call: every row whole
    m = random_matrix(70, 45, 9)
    assert bad_rows(eng.hash_to_field(m, dst=DSTS[1], mode="nu"), want_u_words(m, np.full(70, 45), DSTS[1], "nu")).size == 0


def test_host_calls_over_several_chunks_equal_the_dev_forms(eng):
    """The host-array calls cut into chunks (the message matrix and the lengths are two of a chunk's arrays) against the _dev forms on the
    same bytes, which the tests around this one pin against the restatement.  One chunk of hash_to_field is 16 x lanes rows, so it
    takes more than 2 x lanes + 77 rows to make a second one; one of hash_to_curve is `lanes` rows."""
    import torch
    dev = torch.device("cuda", 0)
    for what, n, stride in (("field", 16 * eng.lanes + 77, 16), ("curve", 2 * eng.lanes + 77, 40)):
        m = random_matrix(n, stride, 31)
        lens = np.random.default_rng(32).integers(0, stride + 1, size=n, dtype=np.uint32)
        d_m, d_lens = torch.from_numpy(m).to(dev), torch.from_numpy(lens.view(np.int32)).to(dev)
        if what == "field":
            got = eng.hash_to_field(m, lens, dst=DSTS[43], mode="nu")
            chunks = eng.host_stats()["chunks"]
            out = torch.empty((n, 1, 4), dtype=torch.int64, device=dev)
            eng.hash_to_field_dev(d_m, stride, d_lens, 0, out, n, dst=DSTS[43], mode="nu")
            eng.sync()
            same = np.array_equal(got, out.cpu().numpy().view(np.uint64))
        else:
            got = eng.hash_to_curve(m, lens, dst=DSTS[43])
            chunks = eng.host_stats()["chunks"]
            out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            eng.hash_to_curve_dev(d_m, stride, d_lens, 0, out, n, dst=DSTS[43])
            eng.sync()
            same = np.array_equal(got, out.cpu().numpy())
        assert chunks > 1 and same, what


# ---- 2. the map -------------------------------------------------------------------------------------------------------------------------
def test_map_to_curve_and_the_primitive(eng):
    rng = random.Random(20261017)
    special = [u for u, _ in ref.special_inputs()]
    assert len(special) == 2
    us = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (P - 1, P - 1), (1, 2)] + special + [(rng.randrange(P), rng.randrange(P)) for _ in range(1000)]
    expect = words([ref.affine_words(want_map(u)) for u in us])
    assert want_map((1, 2)) == ((0x63eae08f8a36f8c839f8c8a88255414, 0x188050f38adcdd8c58d393693ff498f8),
                                (0x6baf5ddc6d5a7d79b22a0aff7c788a8, 0x2beed4aaa95034951838f9089eb0b8e6))
    canonical = words([ref.u_words(u) for u in us])
    shifted = words([ref.u_words((u[0] + P, u[1] + P)) for u in us])              # the same residues as non-canonical words, below 2^128
    for label, u in (("canonical", canonical), ("u + p", shifted)):
        got = eng.map_to_curve(u)
        assert bad_rows(got, expect).size == 0, (label, bad_rows(got, expect)[:8])
        got = eng.prim("PT_MAP_ELL2", u)
        assert bad_rows(got, expect).size == 0, (label, "primitive", bad_rows(got, expect)[:8])
    both = {ref.map_to_montgomery(u)[2] for u in us[:40]}
    assert both == {1, 2}
    assert eng.map_to_curve(np.zeros((0, 4), dtype=np.uint64)).shape == (0, 8)


# ---- 3. hash_to_curve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ro", "nu"])
def test_hash_to_curve_batch_sizes(eng, mode):
    """n = 1, 63, 64, 65, 257 and 4 096 rows of mixed lengths, as bytes and as affine words: every output against the restatement."""
    m, lens = mixed_batch()
    dst = DSTS[43]
    expect32, expect_aff = want_bytes(m, lens, dst, mode), want_affine_words(m, lens, dst, mode)
    for n in SIZES:
        got = eng.hash_to_curve(m[:n], lens[:n], dst=dst, mode=mode)
        assert got.shape == (n, 32) and bad_rows(got, expect32[:n]).size == 0, (n, bad_rows(got, expect32[:n])[:8])
        got = eng.hash_to_curve(m[:n], lens[:n], dst=dst, mode=mode, affine=True)
        assert got.shape == (n, 8) and bad_rows(got, expect_aff[:n]).size == 0, (n, bad_rows(got, expect_aff[:n])[:8])
    assert eng.hash_to_curve(np.zeros((0, 16), dtype=np.uint8), dst=dst, mode=mode).shape == (0, 32)


def test_golden_rows_and_the_bytes_module(eng, golden):
    from fourq_amd import codec
    cases = golden("h2c.json", raw=True)["rows"]
    for dst_hex in sorted({c["dst"] for c in cases}):
        for mode in ("ro", "nu"):
            sel = [c for c in cases if c["dst"] == dst_hex and c["mode"] == mode]
            matrix, lens = codec.pack_messages([bytes.fromhex(c["msg"]) for c in sel])
            got = eng.hash_to_curve(matrix, lens, dst=bytes.fromhex(dst_hex), mode=mode)
            assert [r.tobytes().hex() for r in got] == [c["point"] for c in sel], (len(dst_hex) // 2, mode)
    # three empty messages through a matrix without columns
    empty = eng.hash_to_curve(np.zeros((3, 0), dtype=np.uint8), dst=DSTS[1])
    assert all(r.tobytes() == ref.hash_to_curve(b"", DSTS[1]) for r in empty)


def test_dst_and_mode_separate_every_output(eng):
    m, lens = mixed_batch()
    m, lens = m[:257], lens[:257]
    base = eng.hash_to_curve(m, lens, dst=DSTS[43], mode="ro")
    for other in (eng.hash_to_curve(m, lens, dst=DSTS[43][:-1] + b"!", mode="ro"), eng.hash_to_curve(m, lens, dst=DSTS[43][:-1], mode="ro"),
                  eng.hash_to_curve(m, lens, dst=DSTS[43], mode="nu")):
        assert bad_rows(other, base).size == 257
    u_ro, u_nu = eng.hash_to_field(m, lens, dst=DSTS[43], mode="ro"), eng.hash_to_field(m, lens, dst=DSTS[43], mode="nu")
    assert bad_rows(u_ro[:, 0], u_nu[:, 0]).size == 257                          # len_in_bytes is part of b_0


def test_bad_dst_and_mode_are_refused(eng):
    m = random_matrix(4, 32, 8)
    for dst in (b"", bytes(256)):
        for call in (eng.hash_to_curve, eng.hash_to_field):
            with pytest.raises(FourQError):
                call(m, dst=dst)
        import torch
        d_m = torch.from_numpy(m).to("cuda:0")
        out = torch.empty((4, 64), dtype=torch.uint8, device="cuda:0")
        for call in (eng.hash_to_curve_dev, eng.hash_to_field_dev):
            with pytest.raises(FourQError):
                call(d_m, 32, None, 32, out, 4, dst=dst)
    assert eng.hash_to_curve(m, dst=bytes(255)).shape == (4, 32)
    with pytest.raises(ValueError):
        eng.hash_to_curve(m, dst=b"x", mode="xof")
    with pytest.raises(FourQError):
        eng.hash_to_curve(m, np.array([1, 2, 33, 4], dtype=np.uint32), dst=b"x")      # a length beyond the stride


# ---- 4. a reserved context only enqueues ------------------------------------------------------------------------------------------------
def test_hash_to_curve_dev_can_be_captured_into_a_hip_graph(eng):
    import torch
    dev = torch.device("cuda", 0)
    n = 257
    m, lens = mixed_batch()
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.int32)).to(dev)
    d_m, d_len = to_dev(m[:n]), to_dev(lens[:n])
    out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    try:
        eng.reserve(n)
        eng.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            eng.hash_to_curve_dev(d_m, m.shape[1], d_len, 0, out, n, dst=DSTS[43], mode="ro")
            graph.capture_end()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert bad_rows(out.cpu().numpy(), want_bytes(m[:n], lens[:n], DSTS[43], "ro")).size == 0
        d_m.copy_(to_dev(m[n:2 * n])); d_len.copy_(to_dev(lens[n:2 * n]))        # new rows in the captured buffers
        graph.replay()
        torch.cuda.synchronize()
        assert bad_rows(out.cpu().numpy(), want_bytes(m[n:2 * n], lens[n:2 * n], DSTS[43], "ro")).size == 0
    finally:
        eng.set_stream(None)


# ---- 5. several devices -----------------------------------------------------------------------------------------------------------------
def test_multi_engine(eng):
    from fourq_amd import MultiEngine, device_count
    m, lens = mixed_batch()
    count = device_count()
    with MultiEngine(list(range(count)) if count > 1 else [0, 0]) as multi:
        multi.ct_select = eng.ct_select
        for mode in ("ro", "nu"):
            assert np.array_equal(multi.hash_to_curve(m, lens, dst=DSTS[43], mode=mode), eng.hash_to_curve(m, lens, dst=DSTS[43], mode=mode))
        assert np.array_equal(multi.hash_to_curve(m[:65], lens[:65], dst=DSTS[1], affine=True), eng.hash_to_curve(m[:65], lens[:65], dst=DSTS[1], affine=True))


# ---- 6. the C ABI from C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_c_host_program(eng, tmp_path):
    from fourq_amd.build import LIB_PATH
    src = os.path.join(ROOT, "tests", "c", "h2c_check.c")
    exe, libdir = str(tmp_path / "h2c_check"), os.path.dirname(LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                    "-L", libdir, "-lfourq_amd", "-Wl,-rpath," + libdir], check=True)
    m, lens = mixed_batch()
    n, dst = 257, DSTS[43]
    m, lens = m[:n], lens[:n]
    path = tmp_path / "vectors.bin"
    with open(path, "wb") as fh:
        for v in (n, 1 if eng.ct_select else 0, m.shape[1], len(dst)):
            fh.write(np.uint64(v).tobytes())
        fh.write(dst + bytes(256 - len(dst)))
        fh.write(m.tobytes())
        fh.write(lens.astype("<u4").tobytes())
        for mode in ("ro", "nu"):
            fh.write(want_u_words(m, lens, dst, mode).astype("<u8").tobytes())
            fh.write(want_affine_words(m, lens, dst, mode).astype("<u8").tobytes())
            fh.write(want_bytes(m, lens, dst, mode).tobytes())
        fh.write(words([ref.affine_words(want_map(want_u(m[i, :lens[i]].tobytes(), dst, "nu")[0])) for i in range(n)]).astype("<u8").tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")     # no PyTorch in a C program: the system HIP runtime
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "rows bit-exact through the C ABI" in proc.stdout
