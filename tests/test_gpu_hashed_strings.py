"""Every call that hashes a row of per-lane length, at the row lengths where laying the string into SHA-512 blocks can go wrong: against
the Python restatements the calls' own tests use (hashlib, sig_ref, keyset_ref, h2c_ref, oprf_ref, vrf_ref), computed once per process.
One batch per call and stride with one row per length: 0, 1, 7, 8, 9, 15, 16, 17 and, for the call's own prefix p and tail t, every L with
p + L + t + 17 in {128 k - 1, 128 k, 128 k + 1}, k = 1, 2, 3 -- the padded string ends one byte short of a block, on it, one byte past it.
Strides 320, 328 and 321 take the 16-byte, the 8-byte and the byte-wise loads; DSTs of 1 and 255 bytes the shortest and the longest tail.
The bytes behind each row's length hold a pattern that a second run changes: no output may move, so nothing behind a length is hashed."""
import hashlib

import numpy as np
import pytest

import h2c_ref
import keyset_ref
import oprf_ref
import sig_ref
import vrf_ref
from fourq_amd import codec
from test_gpu_sig import bad_rows, byte_rows, g_comb

pytestmark = pytest.mark.gpu

STRIDES = (320, 328, 321)                   # multiples of 16, of 8 only, of neither: SHA_LOAD_16, SHA_LOAD_8, SHA_LOAD_BYTES
DSTS = (b"D", bytes(range(1, 256)))
FILLS = (0xA5, 0x3C)
BLIND = 0x1234567
_cache = {}


def lengths(prefixes, tail):
    """the row lengths of one batch: `prefixes` the bytes in front of the row in each string of the call that holds it"""
    out = {0, 1, 7, 8, 9, 15, 16, 17}
    for p in prefixes:
        out |= {128 * k + e - 17 - p - tail for k in (1, 2, 3) for e in (-1, 0, 1)}
    return sorted(x for x in out if 0 <= x <= min(STRIDES))


def messages(prefixes, tail, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lengths(prefixes, tail)]


def matrix(msgs, stride, fill):
    m = np.full((len(msgs), stride), fill, dtype=np.uint8)
    for i, s in enumerate(msgs):
        m[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return m, np.array([len(s) for s in msgs], dtype=np.uint32)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int64) if a.dtype == np.uint64 else a
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def out_rows(n, width, dtype=None):
    import torch
    return torch.full((n, width) if width else (n,), 7, dtype=dtype or torch.uint8, device=torch.device("cuda", 0))


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def keys():
    def make():
        sks = [bytes([i]) * 32 for i in (1, 2)]
        return sks, [sig_ref.keygen(sk) for sk in sks]
    return cached("keys", make)


def each_layout(eng, run, want):
    """run(stride, fill) -> arrays; every stride and both fills give `want`"""
    for stride in STRIDES:
        for fill in FILLS:
            got = run(stride, fill)
            eng.sync()
            for g, w in zip(got, want):
                assert bad_rows(host(g), w).size == 0, (stride, fill, bad_rows(host(g), w))


def test_sha512(eng):
    msgs = messages([0], 0, 1)
    want = byte_rows([hashlib.sha512(s).digest() for s in msgs], 64)

    def run(stride, fill):
        m, lens = matrix(msgs, stride, fill)
        out = out_rows(len(msgs), 64)
        eng.sha512_dev(dev(m), stride, dev(lens), 0, out, len(msgs))
        return [out]
    each_layout(eng, run, [want])


def test_sign_then_verify_and_keyed_verify_on_two_registered_keys(eng):
    g_comb(eng)
    msgs = messages([32, 64], 0, 2)             # the nonce's string k[32:64] || msg and the challenge's R || pk || msg
    n = len(msgs)
    sks, pks = keys()
    ids = np.arange(n, dtype=np.uint32) % 2

    def make():
        sigs = [sig_ref.sign(sks[i], pks[i], s) for i, s in zip(ids, msgs)]
        plain = [sig_ref.verify(pks[i], s, sig) for i, s, sig in zip(ids, msgs, sigs)]
        keyed = [keyset_ref.verify_keyed(pks, int(i), s, sig) for i, s, sig in zip(ids, msgs, sigs)]
        assert plain == [(1, 0)] * n and keyed == plain
        return byte_rows(sigs, 64), np.array([r[0] for r in plain], dtype=np.uint8), np.array([r[1] for r in plain], dtype=np.uint8)
    sigs, ok, st = cached("sig", make)
    assert not eng.keyset_set(byte_rows(pks, 32)).any()
    d_sk, d_pk, d_ids = dev(byte_rows([sks[i] for i in ids], 32)), dev(byte_rows([pks[i] for i in ids], 32)), dev(ids)

    def run(stride, fill):
        m, lens = matrix(msgs, stride, fill)
        d_m, d_lens = dev(m), dev(lens)
        sig, ok1, st1, ok2, st2 = out_rows(n, 64), out_rows(n, 0), out_rows(n, 0), out_rows(n, 0), out_rows(n, 0)
        eng.sig_sign_dev(d_sk, d_pk, d_m, stride, d_lens, 0, sig, n)
        eng.sig_verify_dev(d_pk, d_m, stride, d_lens, 0, sig, ok1, st1, n)
        eng.sig_verify_keyed_dev(d_ids, d_m, stride, d_lens, 0, sig, ok2, st2, n)
        return [sig, ok1, st1, ok2, st2]
    each_layout(eng, run, [sigs, ok, st, ok, st])


@pytest.mark.parametrize("mode", ["ro", "nu"])
def test_hash_to_field(eng, mode):
    count = 2 if mode == "ro" else 1
    for dst in DSTS:
        msgs = messages([0], 3 + len(dst) + 1, 3)           # behind Z_pad, a whole block: msg || I2OSP(len_in_bytes, 2) || 0x00 || DST_prime
        want = cached(("h2f", mode, dst), lambda: np.array(
            [[h2c_ref.u_words(u) for u in h2c_ref.hash_to_field(s, dst, h2c_ref.RO if mode == "ro" else h2c_ref.NU)] for s in msgs], dtype=np.uint64))

        def run(stride, fill):
            import torch
            m, lens = matrix(msgs, stride, fill)
            out = torch.full((len(msgs), count, 4), 7, dtype=torch.int64, device=torch.device("cuda", 0))
            eng.hash_to_field_dev(dev(m), stride, dev(lens), 0, out, len(msgs), dst=dst, mode=mode)
            return [out]
        each_layout(eng, run, [want])


def test_oprf_finalize(eng):
    z32 = keys()[1][0]                                      # any point of order N as the evaluated element
    for dst in DSTS:
        msgs = messages([32], 8 + len(dst) + 1, 4)          # E || msg || "Finalize" || DST || I2OSP(len(DST), 1)
        n = len(msgs)
        rows = cached(("oprf", dst), lambda: [oprf_ref.finalize(s, dst, BLIND, z32) for s in msgs])
        want = byte_rows([r[0] for r in rows], 64), np.array([r[1] for r in rows], dtype=np.uint8)
        assert not want[1].any()
        d_r, d_z = dev(codec.pack_scalars([BLIND] * n)), dev(byte_rows([z32] * n, 32))

        def run(stride, fill):
            m, lens = matrix(msgs, stride, fill)
            out, st = out_rows(n, 64), out_rows(n, 0)
            eng.oprf_finalize_dev(dev(m), stride, dev(lens), 0, d_r, d_z, out, st, n, dst=dst)
            return [out, st]
        each_layout(eng, run, want)


def test_vrf_prove_then_verify(eng):
    g_comb(eng)
    sks, pks = keys()
    for dst in DSTS:
        msgs = messages([32], 3 + len(dst) + 1, 5)          # behind Z_pad: pk32 || alpha || I2OSP(128, 2) || 0x00 || DST_prime
        n = len(msgs)

        def make():
            proofs = [vrf_ref.prove(sks[i % 2], pks[i % 2], s, dst) for i, s in enumerate(msgs)]
            checked = [vrf_ref.verify(pks[i % 2], s, p, dst) for i, (s, p) in enumerate(zip(msgs, proofs))]
            assert all(r[0] == 1 and r[1] == 0 for r in checked)
            return byte_rows(proofs, 96), byte_rows([r[2] for r in checked], 64)
        proofs, betas = cached(("vrf", dst), make)
        d_sk, d_pk = dev(byte_rows([sks[i % 2] for i in range(n)], 32)), dev(byte_rows([pks[i % 2] for i in range(n)], 32))

        def run(stride, fill):
            m, lens = matrix(msgs, stride, fill)
            d_m, d_lens = dev(m), dev(lens)
            proof, beta, ok, st = out_rows(n, 96), out_rows(n, 64), out_rows(n, 0), out_rows(n, 0)
            eng.vrf_prove_dev(d_sk, d_pk, d_m, stride, d_lens, 0, proof, n, dst=dst)
            eng.vrf_verify_dev(d_pk, d_m, stride, d_lens, 0, proof, beta, ok, st, n, dst=dst)
            return [proof, beta, ok, st]
        each_layout(eng, run, [proofs, betas, np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)])
