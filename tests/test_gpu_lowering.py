"""The lowering kernels at the size where their K switches, at every residue of n modulo K (fourq_amd/csrc/lower.hip.h: lane t owns
elements t, t + T, ..., t + (K-1) T with T = ceil(n / K)).  With L = eng.lanes a device-resident batch beyond 2 L rows runs
lower_kernel<4, *> behind MUL_endo and combine_kernel<2, *> behind [k]B + [l]P; the other tests of these kernels use one n each.

Row i carries pair i mod 61 of 61 distinct seeded rows, so the slots of one lane hold different pairs.  Expected values: the C oracle on
the 61 rows (for the double multiplication its two halves joined by the Python oracle's ADD, as tests/test_gpu_double_mul.py), tiled and
compared on EVERY row.  Poisoned rows -- the all-zero pair for the affine calls, a string the reference's decode refuses (tests/golden/wire.json)
for the byte calls -- sit at ids 0, T - 1, T and n - 1: the first and last lane's first slots, the first lane's second slot, the ragged end.
They get (0, 0), a zero row with BYTES_DECODE_BASE + code, or ok = 0, and every other row is what it is without them."""
import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_scalars
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu

PAIRS = 61
G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
CODE = {"Malformed point: reserved bit is not zero": _lib.DECODE_RESERVED_BIT, "Point not on curve": _lib.DECODE_NOT_ON_CURVE,
        "type object 'GFp' has no attribute 'two'": _lib.DECODE_REF_ATTRIBUTE_ERROR}
_cache = {}


def _lift(aff):
    r1 = np.zeros((len(aff), 20), dtype=np.uint64)
    r1[:, 0:8] = aff
    r1[:, 8] = 1
    r1[:, 12:20] = aff
    return r1


def _rows():
    """The 61 rows and what the oracle makes of them; computed once, never written to."""
    if "rows" not in _cache:
        table = oc.table(oc.ENDO, G1_WORDS)
        s, k, l = seeded_scalars(6101, PAIRS), seeded_scalars(6102, PAIRS), seeded_scalars(6103, PAIRS)
        aff = oc.r1_to_affine(oc.mul(oc.ENDO, seeded_scalars(6104, PAIRS), None, table))           # 61 points [t_i]G
        assert len({bytes(r) for r in aff}) == PAIRS and len({bytes(r) for r in s}) == PAIRS
        mul_aff = oc.r1_to_affine(oc.mul(oc.ENDO, s, _lift(aff)))
        first = codec.unpack_points(oc.mul(oc.ENDO, k, None, table))
        second = codec.unpack_points(oc.mul(oc.ENDO, l, _lift(aff)))
        dm_aff = oc.r1_to_affine(codec.pack_points([o.ADD(A, o.R1toR2(B)) for A, B in zip(first, second)], 5))
        r = dict(s=s, k=k, l=l, aff=aff, keys=oc.encode(aff), mul_aff=mul_aff, mul_enc=oc.encode(mul_aff), dm_aff=dm_aff, dm_enc=oc.encode(dm_aff))
        for a in r.values():
            a.setflags(write=False)
        _cache["rows"] = r
    return _cache["rows"]


def _refused(golden):
    """(32 bytes, status the byte calls report) of strings the reference's decode refuses"""
    rows = [r for r in golden("wire.json", raw=True)["strings"] if r[1] != "ok"]
    assert len(rows) >= 4
    return [(np.frombuffer(bytes.fromhex(r[0]), dtype=np.uint8), _lib.BYTES_DECODE_BASE + CODE[r[2]]) for r in rows]


def _poisoned(n, K):
    T = (n + K - 1) // K
    at = sorted({0, T - 1, T, n - 1})
    assert len(at) == 4
    return at


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def _empty(shape, dtype):
    import torch
    return torch.empty(shape, dtype=dtype, device=torch.device("cuda", 0))


def _bad_rows(got, want):
    return np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))[:8]


@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_lower_kernel_4_at_every_residue(eng, golden, r):
    import torch
    rows, n = _rows(), 2 * eng.lanes + r
    idx = np.arange(n) % PAIRS
    at = _poisoned(n, 4)
    s = rows["s"][idx]
    # affine words in and out: the all-zero pair gives (0, 0)
    aff, want = rows["aff"][idx], rows["mul_aff"][idx]
    aff[at] = 0
    want[at] = 0
    out = _empty((n, 8), torch.int64)
    eng.mul_affine_dev(_to_dev(s), _to_dev(aff), out, n)
    eng.sync()
    got = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), _bad_rows(got, want)
    # 32 bytes in and out: a refused string gives a zero row and its decode code
    keys, want, want_st = rows["keys"][idx], rows["mul_enc"][idx], np.zeros(n, dtype=np.uint8)
    for i, (string, status) in zip(at, _refused(golden)):
        keys[i], want[i], want_st[i] = string, 0, status
    out, st = _empty((n, 32), torch.uint8), _empty(n, torch.uint8)
    eng.mul_bytes_dev(_to_dev(s), _to_dev(keys), out, st, n)
    eng.sync()
    got, st = out.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, want_st), np.flatnonzero(st != want_st)[:8]
    assert np.array_equal(got, want), _bad_rows(got, want)


@pytest.mark.parametrize("r", [1, 2])
def test_combine_kernel_2_at_every_residue(eng, golden, r):
    import torch
    rows, n = _rows(), 2 * eng.lanes + r
    idx = np.arange(n) % PAIRS
    at = _poisoned(n, 2)
    eng.comb_stage(_cache.setdefault("comb", eng.comb_table(G1_WORDS)))
    k, l = _to_dev(rows["k"][idx]), _to_dev(rows["l"][idx])
    aff, want = rows["aff"][idx], rows["dm_aff"][idx]
    aff[at] = 0
    want[at] = 0
    out = _empty((n, 8), torch.int64)
    eng.double_mul_dev(k, l, _to_dev(aff), out, n)
    eng.sync()
    got = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), _bad_rows(got, want)
    keys, want, want_st, want_ok = rows["keys"][idx], rows["dm_enc"][idx], np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)
    expect = want.copy()
    for i, (string, status) in zip(at, _refused(golden)):
        keys[i], want[i], want_st[i], want_ok[i] = string, 0, status, 0
    out, st = _empty((n, 32), torch.uint8), _empty(n, torch.uint8)
    eng.double_mul_bytes_dev(k, l, _to_dev(keys), out, st, n)
    eng.sync()
    got, st = out.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, want_st), np.flatnonzero(st != want_st)[:8]
    assert np.array_equal(got, want), _bad_rows(got, want)
    ok, st = _empty(n, torch.uint8), _empty(n, torch.uint8)
    eng.verify_bytes_dev(k, l, _to_dev(keys), _to_dev(expect), ok, st, n)
    eng.sync()
    ok, st = ok.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(ok, want_ok), np.flatnonzero(ok != want_ok)[:8]
    assert np.array_equal(st, want_st), np.flatnonzero(st != want_st)[:8]
