"""A context's FIRST protocol call, at n = 257, on a newly created Engine: no reserve, nothing called before it except staging the comb.
On a fresh context every ensure_work inside the call really allocates, so a layout whose total and carving disagreed
(fourq_amd/csrc/work_layout.h) would write past the buffer here; n = 257 is the smallest size at which align256(n) != n and a status
region spills into a second 256-byte unit.  Expected values: tests/sig_ref.py and the C oracle, as the neighbouring tests."""
import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
import sig_ref as ref
from bench import seeded_scalars
from fourq_amd import Engine, codec

pytestmark = pytest.mark.gpu

N_FIRST = 257
_cache = {}


@pytest.fixture
def fresh():
    """A new context with G's comb staged; the table itself (data) comes from a context that is gone again."""
    if "comb" not in _cache:
        with Engine(0) as helper:
            _cache["comb"] = helper.comb_table(codec.pack_point(ref.G1))
    e = Engine(0)
    e.comb_stage(_cache["comb"])
    yield e
    e.close()


def signed_batch():
    if "sig" not in _cache:
        sk = np.random.default_rng(7257).integers(0, 256, size=(N_FIRST, 32), dtype=np.uint8)
        sks = [r.tobytes() for r in sk]
        msgs = [bytes([i & 255]) * (i % 131) for i in range(N_FIRST)]              # 0 .. 130 bytes: one and two hash blocks
        pks = ref.batch_keygen(sks)
        _cache["sig"] = (sk, msgs, pks, ref.batch_sign(sks, pks, msgs))
    return _cache["sig"]


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def dev_empty(*shape):
    import torch
    return torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", 0))


def test_first_call_sig_verify_dev(fresh):
    _, msgs, pks, sigs = signed_batch()
    sigs = sigs.copy()
    want_ok = np.ones(N_FIRST, dtype=np.uint8)
    for i in (0, 128, 255, 256):                                                   # the last row of each 256-byte status unit among them
        sigs[i, 5] ^= 1
        want_ok[i], st = ref.verify(pks[i].tobytes(), msgs[i], sigs[i].tobytes())
        assert (want_ok[i], st) == (0, 0)
    matrix, lens = codec.pack_messages(msgs)
    ok, st = dev_empty(N_FIRST), dev_empty(N_FIRST)
    fresh.sig_verify_dev(to_dev(pks), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, to_dev(sigs), ok, st, N_FIRST)
    fresh.sync()
    assert np.array_equal(ok.cpu().numpy(), want_ok) and not st.cpu().numpy().any()


def test_first_call_sig_sign_dev(fresh):
    sk, msgs, pks, sigs = signed_batch()
    matrix, lens = codec.pack_messages(msgs)
    out = dev_empty(N_FIRST, 64)
    fresh.sig_sign_dev(to_dev(sk), to_dev(pks), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, out, N_FIRST)
    fresh.sync()
    assert np.array_equal(out.cpu().numpy(), sigs)


def test_first_call_double_mul_bytes_dev(fresh):
    # [k]G + [l]([t]G) = [(k + l t) mod N]G, the point work in the C oracle
    k, l, t = seeded_scalars(7301, N_FIRST), seeded_scalars(7302, N_FIRST), seeded_scalars(7303, N_FIRST)
    table = oc.table(oc.ENDO, codec.pack_point(ref.G1))
    sums = [(x + y * z) % o.N for x, y, z in zip(codec.unpack_scalars(k), codec.unpack_scalars(l), codec.unpack_scalars(t))]
    want = oc.encode(oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, table)))
    keys = oc.encode(oc.r1_to_affine(oc.mul(oc.ENDO, t, None, table))).copy()
    out, st = dev_empty(N_FIRST, 32), dev_empty(N_FIRST)
    fresh.double_mul_bytes_dev(to_dev(k), to_dev(l), to_dev(keys), out, st, N_FIRST)
    fresh.sync()
    assert not st.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), want)
