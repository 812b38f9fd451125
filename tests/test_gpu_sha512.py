"""SHA-512 on the device (fourq_sha512_batch / _dev, sha512.hip.h) against hashlib: every block-count boundary, every row alignment,
divergent lengths inside a wave, and no byte behind a row's length ever entering a digest."""
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def want(matrix, lens):
    return np.frombuffer(b"".join(hashlib.sha512(matrix[i, :lens[i]].tobytes()).digest() for i in range(len(matrix))), dtype=np.uint8).reshape(-1, 64)


def random_matrix(n, stride, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, stride), dtype=np.uint8)


def bad_rows(got, expect):
    return np.flatnonzero((got != expect).any(axis=1))


def test_every_length_up_to_300_in_one_call(eng):
    """Rows of 0 .. 300 bytes side by side: lanes of one wave run one, two or three blocks."""
    lens = np.arange(301, dtype=np.uint32)
    m = random_matrix(301, 304, 1)
    got = eng.sha512(m, lens)
    assert bad_rows(got, want(m, lens)).size == 0, bad_rows(got, want(m, lens))[:8]
    order = np.random.default_rng(2).permutation(301)
    assert np.array_equal(eng.sha512(m[order], lens[order]), got[order])


def test_long_messages(eng):
    for length in (1000, 65537):
        m = random_matrix(5, length + 7, length)
        lens = np.array([length, length - 1, length, 0, length - 129], dtype=np.uint32)
        assert np.array_equal(eng.sha512(m, lens), want(m, lens)), length


def test_every_stride_alignment(eng):
    """stride % 16 = 0 .. 15 with a 16-byte aligned base: rows start at every alignment; 16-byte, 8-byte and byte loads."""
    rng = random.Random(3)
    for stride in range(144, 160):
        m = random_matrix(130, stride, stride)
        lens = np.array([rng.randrange(stride + 1) for _ in range(130)], dtype=np.uint32)
        lens[:3] = (stride, 0, stride - 1)
        got = eng.sha512(m, lens)
        assert bad_rows(got, want(m, lens)).size == 0, (stride, bad_rows(got, want(m, lens))[:8])


def test_dev_form_on_an_offset_view(eng):
    """The _dev call on a matrix that starts 16 bytes into an allocation, every stride alignment, lengths from the device."""
    import torch
    dev = torch.device("cuda", 0)
    rng = random.Random(4)
    for stride in (37, 40, 48, 129):
        n = 200
        m = random_matrix(n, stride, 1000 + stride)
        lens = np.array([rng.randrange(stride + 1) for _ in range(n)], dtype=np.uint32)
        buf = torch.zeros(16 + n * stride, dtype=torch.uint8, device=dev)
        buf[16:] = torch.from_numpy(m.reshape(-1)).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
        out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        eng.sha512_dev(buf.data_ptr() + 16, stride, d_lens, 0, out, n)
        eng.sync()
        assert np.array_equal(out.cpu().numpy(), want(m, lens)), stride
        # lens = NULL: every row is msg_len bytes
        eng.sha512_dev(buf.data_ptr() + 16, stride, None, stride - 5, out, n)
        eng.sync()
        assert np.array_equal(out.cpu().numpy(), want(m, np.full(n, stride - 5))), stride
        # a length above the stride is clamped to it (the _dev calls cannot refuse it)
        over = lens.copy()
        over[::3] = stride + 9
        eng.sha512_dev(buf.data_ptr() + 16, stride, torch.from_numpy(over.view(np.int32)).to(dev), 0, out, n)
        eng.sync()
        assert np.array_equal(out.cpu().numpy(), want(m, np.minimum(over, stride))), stride


def test_fixed_length_and_batch_sizes(eng):
    for n in (1, 255, 256, 257, 1 << 16):
        m = random_matrix(n, 112, n)
        got = eng.sha512(m)                                   # lens = NULL, msg_len = the row
        if n <= 257:
            assert np.array_equal(got, want(m, np.full(n, 112))), n
        else:
            expect = want(m, np.full(n, 112))
            assert bad_rows(got, expect).size == 0, bad_rows(got, expect)[:8]
    assert eng.sha512(np.zeros((0, 16), dtype=np.uint8)).shape == (0, 64)
    empty = eng.sha512(np.zeros((3, 0), dtype=np.uint8))      # stride 0: three empty messages
    assert all(r.tobytes() == hashlib.sha512(b"").digest() for r in empty)


def test_bytes_behind_a_rows_length_do_not_reach_the_digest(eng):
    rng = random.Random(5)
    for stride in (160, 168, 163):
        lens = np.array([rng.randrange(stride + 1) for _ in range(512)], dtype=np.uint32)
        a, b = random_matrix(512, stride, 6), random_matrix(512, stride, 7)
        for i, ln in enumerate(lens):
            b[i, :ln] = a[i, :ln]                             # same messages, different bytes behind them
        ga, gb = eng.sha512(a, lens), eng.sha512(b, lens)
        assert np.array_equal(ga, gb) and np.array_equal(ga, want(a, lens)), stride


def test_host_call_refuses_lengths_beyond_the_stride(eng):
    from fourq_amd import FourQError
    m = random_matrix(4, 32, 8)
    with pytest.raises(FourQError):
        eng.sha512(m, np.array([1, 2, 33, 4], dtype=np.uint32))


def test_host_call_over_several_chunks_equals_the_dev_form(eng):
    """The host-array call cut into chunks (the message matrix and the lengths are two of the chunk's arrays) against the _dev form on
    the same bytes, which the tests above pin against hashlib.  One chunk of this call is 16 x lanes rows, so it takes more than
    2 x lanes + 77 rows to make a second one."""
    import torch
    dev = torch.device("cuda", 0)
    n, stride = 16 * eng.lanes + 77, 16
    m = random_matrix(n, stride, 9)
    lens = np.random.default_rng(10).integers(0, stride + 1, size=n, dtype=np.uint32)
    got = eng.sha512(m, lens)
    assert eng.host_stats()["chunks"] > 1
    out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    eng.sha512_dev(torch.from_numpy(m).to(dev), stride, torch.from_numpy(lens.view(np.int32)).to(dev), 0, out, n)
    eng.sync()
    assert np.array_equal(got, out.cpu().numpy())
