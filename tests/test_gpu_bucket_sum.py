"""The grouped sums by the bucket method on the device (fourq_bucketsum_*, fourq_amd/csrc/bucket.hip.h): byte for byte what fourq_msm_* gives.

Expected values never come from the code under test: the group law  sum [k_i][t_i]G = [(sum k_i t_i) mod N]G  with the modular arithmetic in
Python integers and the point work in the C oracle, and, for points outside the order-N subgroup, the Python oracle's ADD chained over the C
oracle's MUL_endo rows.  tests/test_bucket_oracle.py pins the identity behind the route on the CPU.  Every test takes `eng`: with table
selection by address the bucket route runs; with constant-time selection the library falls back to the ladder route, same expectations.

Window 4 has 15 buckets per column, the smallest at which every pass boundary is reachable: a bucket's rows are cut into parts of 64, so
group sizes 63, 64, 65 and 64^2 + 1 = 4097 are where a second and a third accumulation pass start.  Elements handed to the calls under test
across this file: about 120 000 (the shapes 72 702, the hot buckets 41 200, the window sweep 3 600, the rest under 3 000)."""
import ctypes

import numpy as np
import pytest

import bucket_ref as ref
import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_scalars
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu

G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
NEUTRAL_AFFINE = codec.pack_points([((0, 0), (1, 0))], 2)[0]
NEUTRAL_ENC = np.frombuffer(bytes([1] + [0] * 31), dtype=np.uint8)
SIZES = [1, 2, 3, 63, 64, 65, 127, 4097]
SHAPES = [(g, s) for s in SIZES for g in ([1, 3, 67] if s <= 65 else [1, 3])]
POOL = 3 * 4097                                                       # the largest shape
SWEEP = [4, 5, 7, 8, 11, 12, 0]                                       # 5, 7, 11, 12 leave a short top window: 65, 70, 66 and 72 bits

_cache = {}


def pool(eng):
    """POOL seeded scalars k (the six edge values planted, bucket_ref.pool_scalars) and points P_i = [t_i]G from the comb call, checked against
    the C oracle.  One per session: both selection modes share it."""
    if "pool" not in _cache:
        table = oc.table(oc.ENDO, G1_WORDS)
        k = ref.pool_scalars(POOL)
        t_words = seeded_scalars(7405, POOL)
        P, st = eng.comb_mul(t_words, eng.comb_table(G1_WORDS))
        assert not st.any()
        assert np.array_equal(P, oc.r1_to_affine(oc.mul(oc.ENDO, t_words, None, table)))
        _cache["pool"] = {"k": k, "t": codec.unpack_scalars(t_words), "k_words": codec.pack_scalars(k), "P": P, "enc": oc.encode(P), "table": table}
    return _cache["pool"]


def multiples_of_g(c, sums):
    """affine words and encodings of [s mod N]G through the C oracle"""
    want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars([s % o.N for s in sums]), None, c["table"]))
    return want, oc.encode(want)


def expected(eng, groups, size):
    key = ("want", groups, size)
    if key not in _cache:
        c = pool(eng)
        _cache[key] = multiples_of_g(c, [sum(c["k"][i] * c["t"][i] for i in range(g * size, (g + 1) * size)) for g in range(groups)])
    return _cache[key]


def mismatches(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def dev_affine(eng, k, P, groups, size, window, sync=True):
    """_dev call into a 0xA5-filled tensor of groups + 2 rows: (the tensor, how to read it once synchronised)"""
    import torch
    out = torch.full((groups + 2, 64), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    keep = (to_dev(k), to_dev(P))
    eng.bucket_sum_dev(keep[0], keep[1], out, groups, size, window)
    read = lambda: out.cpu().numpy().view(np.uint64)
    if not sync:
        return read, keep
    eng.sync()
    got = read()
    assert (got[groups:].view(np.uint8) == 0xA5).all()
    return got[:groups]


def dev_bytes(eng, k, enc, groups, size, window):
    import torch
    dev = torch.device("cuda", 0)
    out = torch.full((groups + 2, 32), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.full((groups + 2,), 0xA5, dtype=torch.uint8, device=dev)
    eng.bucket_sum_bytes_dev(to_dev(k), to_dev(enc), out, st, groups, size, window)
    eng.sync()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert (out[groups:] == 0xA5).all() and (st[groups:] == 0xA5).all()
    return out[:groups], st[:groups]


def check_all_flavours(eng, k, P, enc, groups, size, window, want, want_enc, every=True):
    """affine through the host arrays and bytes through _dev always; with `every` also affine through _dev and bytes through the host arrays"""
    got = eng.bucket_sum(k, P, size, window)
    assert got.shape == (groups, 8) and mismatches(got, want).size == 0, mismatches(got, want)[:8]
    out, st = dev_bytes(eng, k, enc, groups, size, window)
    assert not st.any() and mismatches(out, want_enc).size == 0, mismatches(out, want_enc)[:8]
    if every:
        got = dev_affine(eng, k, P, groups, size, window)
        assert mismatches(got, want).size == 0, mismatches(got, want)[:8]
        out, st = eng.bucket_sum_bytes(k, enc, size, window)
        assert out.shape == (groups, 32) and not st.any() and mismatches(out, want_enc).size == 0, mismatches(out, want_enc)[:8]


# ---- 1. every shape at which a pass starts or ends, window 4 -----------------------------------------------------------------------------
@pytest.mark.parametrize("groups,size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes_at_window_4(eng, groups, size):
    """Affine and bytes, host arrays and _dev, at every shape; the 67-group shapes and 3 x 4097 run affine on the host arrays and bytes
    through _dev only (the other two pairings run at the same sizes with 1 and 3 groups)."""
    c = pool(eng)
    n = groups * size
    want, want_enc = expected(eng, groups, size)
    check_all_flavours(eng, c["k_words"][:n], c["P"][:n], c["enc"][:n], groups, size, 4, want, want_enc, every=groups <= 3 and n < 3 * 4097)


def test_shape_list_is_the_one_promised():
    assert {1, 2, 3, 63, 64, 65, 127, 64 * 64 + 1} == set(SIZES) and len(SHAPES) == 6 * 3 + 2 * 2
    assert all((g, s) in SHAPES for s in SIZES for g in (1, 3)) and all((67, s) in SHAPES for s in SIZES if s <= 65)
    assert 2 * sum(g * s for g, s in SHAPES) + 2 * sum(g * s for g, s in SHAPES if g <= 3 and g * s < 3 * 4097) == 72702


# ---- 2. every window shape: whole windows, short top windows, the library's own choice ------------------------------------------------------
@pytest.mark.parametrize("window", SWEEP)
def test_window_sweep_at_group_size_257(eng, window):
    c = pool(eng)
    want, want_enc = expected(eng, 1, 257)
    check_all_flavours(eng, c["k_words"][:257], c["P"][:257], c["enc"][:257], 1, 257, window, want, want_enc, every=False)
    assert eng.bucket_sum_window(257) in [0] + list(range(4, 13))


# ---- 3. all scalars equal: one bucket per column holds the whole group ------------------------------------------------------------------------
@pytest.mark.parametrize("window", [4, 8])
@pytest.mark.parametrize("rows", [65, 4096, 4097])
def test_hot_bucket(eng, rows, window):
    """4097 = 64^2 + 1 equal scalars on distinct points: a bucket of 4097 rows leaves 65, then 2, then 1 -- three passes; 4096 and 65 stop one
    part short of the next pass.  [k]P_0 + ... + [k]P_(n-1) = [k (t_0 + ... + t_(n-1)) mod N]G."""
    c = pool(eng)
    k = c["k"][11]
    assert all(v != 0 for v in ref.sub_scalars(k))
    k_words = np.tile(codec.pack_scalars([k]), (rows, 1))
    want, want_enc = multiples_of_g(c, [k * sum(c["t"][:rows])])
    got = eng.bucket_sum(k_words, c["P"][:rows], rows, window)
    assert np.array_equal(got, want)
    out, st = dev_bytes(eng, k_words, c["enc"][:rows], 1, rows, window)
    assert not st.any() and np.array_equal(out, want_enc)


@pytest.mark.parametrize("window", [4, 8])
def test_hot_bucket_of_one_repeated_point(eng, window):
    """4097 times the same (scalar, point): every addition inside the bucket is a doubling case of the complete addition"""
    c = pool(eng)
    k, rows = c["k"][12], 4097
    k_words = np.tile(codec.pack_scalars([k]), (rows, 1))
    want, want_enc = multiples_of_g(c, [rows * k * c["t"][5]])
    assert np.array_equal(eng.bucket_sum(k_words, np.tile(c["P"][5], (rows, 1)), rows, window), want)


# ---- 4. everything cancels ------------------------------------------------------------------------------------------------------------------
def test_cancellation_and_all_zero_scalars(eng):
    """Pairs (k, P), (k, -P) fill a group: every bucket and every S_j is the neutral.  Expect (0, 1) / 01 00 .. 00, status 0.  And a group
    whose scalars are all 0."""
    c = pool(eng)
    half = 65
    pts = codec.unpack_points(c["P"][:half])
    neg = codec.pack_points([(o.f2_neg(x), y) for x, y in pts], 2)
    assert all(o.PointOnCurve(p) for p in codec.unpack_points(neg[:3]))
    P = np.concatenate([c["P"][:half], neg])
    k = np.concatenate([c["k_words"][:half], c["k_words"][:half]])
    enc = oc.encode(P)
    for window in (4, 8):
        assert np.array_equal(eng.bucket_sum(k, P, 2 * half, window), NEUTRAL_AFFINE[None, :])
        out, st = eng.bucket_sum_bytes(k, enc, 2 * half, window)
        assert not st.any() and np.array_equal(out, NEUTRAL_ENC[None, :])
        assert np.array_equal(dev_affine(eng, k, P, 1, 2 * half, window), NEUTRAL_AFFINE[None, :])
    zeros = np.zeros((3 * 17, 4), dtype=np.uint64)
    assert np.array_equal(eng.bucket_sum(zeros, c["P"][:51], 17, 4), np.tile(NEUTRAL_AFFINE, (3, 1)))
    out, st = eng.bucket_sum_bytes(zeros, c["enc"][:51], 17, 8)
    assert not st.any() and np.array_equal(out, np.tile(NEUTRAL_ENC, (3, 1)))


# ---- 5. points outside the order-N subgroup: MUL_endo's value, not [k]P ----------------------------------------------------------------------
def test_points_outside_the_subgroup(eng):
    groups, size = 2, 33
    found = ref.outside_subgroup_points(7406, groups * size)
    enc = np.frombuffer(b"".join(e for e, _ in found), dtype=np.uint8).reshape(-1, 32).copy()
    P = codec.pack_points([p for _, p in found], 2)
    k = pool(eng)["k_words"][100:100 + groups * size]
    rows = np.zeros((len(found), 20), dtype=np.uint64)
    rows[:, 0:8], rows[:, 8], rows[:, 12:20] = P, 1, P
    products = codec.unpack_points(oc.mul(oc.ENDO, k, rows))
    want = []
    for g in range(groups):
        acc = products[g * size]
        for B in products[g * size + 1:(g + 1) * size]:
            acc = o.ADD(acc, o.R1toR2(B))
        want.append(bytes(o.encode(*o.R1toAffine(acc))))
    want = np.frombuffer(b"".join(want), dtype=np.uint8).reshape(groups, 32)
    for window in (4, 8):
        out, st = eng.bucket_sum_bytes(k, enc, size, window)
        assert not st.any() and np.array_equal(out, want), window


# ---- 6. encodings that do not decode --------------------------------------------------------------------------------------------------------
def test_undecodable_elements_mark_their_group_only(eng):
    """One bad string, then two with different codes, in the middle group of three: status 16 + the larger code, a zero row, and the
    neighbours equal to their clean values."""
    from test_gpu_msm import refused
    c = pool(eng)
    bad = refused()
    groups, size = 3, 65
    n = groups * size
    want, want_enc = expected(eng, groups, size)
    for cells, window in (([(40, 2)], 4), ([(0, 1), (64, 3)], 4), ([(7, 3), (8, 2)], 8)):
        enc = c["enc"][:n].copy()
        for pos, code in cells:
            enc[size + pos] = bad[code][pos % len(bad[code])]
        code = _lib.BYTES_DECODE_BASE + max(code for _, code in cells)
        for out, st in (eng.bucket_sum_bytes(c["k_words"][:n], enc, size, window), dev_bytes(eng, c["k_words"][:n], enc, groups, size, window)):
            assert list(st) == [0, code, 0], cells
            assert not out[1].any() and np.array_equal(out[[0, 2]], want_enc[[0, 2]]), cells


# ---- 7. the argument rules, reserve, and calls that do not wait for each other ----------------------------------------------------------------
def test_argument_rules(eng):
    import torch
    c = pool(eng)
    lib, ctx, dev = eng._lib, eng._ctx, torch.device("cuda", 0)
    k, P, enc = to_dev(c["k_words"][:16]), to_dev(c["P"][:16]), to_dev(c["enc"][:16])
    out = torch.full((5, 64), 0xA5, dtype=torch.uint8, device=dev)
    out32, st = torch.full((5, 32), 0xA5, dtype=torch.uint8, device=dev), torch.full((6,), 0xA5, dtype=torch.uint8, device=dev)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    affine, bytes_ = lib.fourq_bucketsum_affine_dev, lib.fourq_bucketsum_bytes_dev
    INVALID = _lib.ERR_INVALID
    # NULLs
    assert affine(None, ptr(k), ptr(P), ptr(out), 4, 4, 4) == INVALID
    assert affine(ctx, None, ptr(P), ptr(out), 4, 4, 4) == INVALID and affine(ctx, ptr(k), None, ptr(out), 4, 4, 4) == INVALID
    assert affine(ctx, ptr(k), ptr(P), None, 4, 4, 4) == INVALID
    assert bytes_(None, ptr(k), ptr(enc), ptr(out32), ptr(st), 4, 4, 4) == INVALID
    for hole in range(4):
        args = [ptr(k), ptr(enc), ptr(out32), ptr(st)]
        args[hole] = None
        assert bytes_(ctx, *args, 4, 4, 4) == INVALID, hole
    assert lib.fourq_bucketsum_reserve(None, 4, 4, 4) == INVALID
    # every array pointer 16-byte aligned; status need not be
    assert affine(ctx, ptr(k, 8), ptr(P), ptr(out), 3, 4, 4) == INVALID
    assert affine(ctx, ptr(k), ptr(P, 8), ptr(out), 3, 4, 4) == INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out, 8), 3, 4, 4) == INVALID
    assert bytes_(ctx, ptr(k), ptr(enc, 8), ptr(out32), ptr(st), 3, 4, 4) == INVALID
    # the count and the window
    for window in (1, 3, 13, 255):
        assert affine(ctx, ptr(k), ptr(P), ptr(out), 4, 4, window) == INVALID, window
        assert bytes_(ctx, ptr(k), ptr(enc), ptr(out32), ptr(st), 4, 4, window) == INVALID, window
        assert lib.fourq_bucketsum_reserve(ctx, 4, 4, window) == INVALID, window
        assert lib.fourq_bucketsum_affine(ctx, c["k_words"].ctypes.data, c["P"].ctypes.data, c["P"].ctypes.data, 4, 4, window) == INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 4, 0, 4) == INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 1 << 16, 1 << 16, 4) == INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out), _lib.MAX_BATCH // 2 + 1, 2, 0) == INVALID
    assert bytes_(ctx, ptr(k), ptr(enc), ptr(out32), ptr(st), (1 << 62) + 1, 4, 4) == INVALID
    assert lib.fourq_bucketsum_reserve(ctx, 1 << 16, 1 << 16, 4) == INVALID and lib.fourq_bucketsum_reserve(ctx, 4, 0, 4) == INVALID
    # no groups is no work: nothing is touched
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 0, 4, 4) == _lib.OK and affine(ctx, ptr(k), ptr(P), ptr(out), 0, 0, 0) == _lib.OK
    assert bytes_(ctx, ptr(k), ptr(enc), ptr(out32), ptr(st), 0, 4, 8) == _lib.OK and lib.fourq_bucketsum_reserve(ctx, 0, 4, 4) == _lib.OK
    host_out = np.full((2, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert lib.fourq_bucketsum_affine(ctx, c["k_words"].ctypes.data, c["P"].ctypes.data, host_out.ctypes.data, 0, 3, 4) == _lib.OK
    assert lib.fourq_bucketsum_affine(ctx, c["k_words"].ctypes.data, c["P"].ctypes.data, host_out.ctypes.data, 2, 0, 4) == INVALID
    assert lib.fourq_bucketsum_affine(ctx, None, None, None, 0, 0, 4) == INVALID
    eng.sync()
    assert (host_out == 0xA5A5A5A5A5A5A5A5).all()
    assert (out.cpu().numpy() == 0xA5).all() and (out32.cpu().numpy() == 0xA5).all() and (st.cpu().numpy() == 0xA5).all()
    # ... and a good call writes its `groups` rows and nothing else; an odd status pointer is fine
    assert bytes_(ctx, ptr(k), ptr(enc), ptr(out32), ptr(st, 1), 4, 4, 4) == _lib.OK
    eng.sync()
    want4, want4_enc = multiples_of_g(c, [sum(c["k"][i] * c["t"][i] for i in range(g * 4, g * 4 + 4)) for g in range(4)])
    assert np.array_equal(out32.cpu().numpy()[:4], want4_enc) and (out32.cpu().numpy()[4] == 0xA5).all()
    assert list(st.cpu().numpy()) == [0xA5, 0, 0, 0, 0, 0xA5]
    with pytest.raises(ValueError):
        eng.bucket_sum(c["k_words"][:7], c["P"][:7], 2, 4)
    with pytest.raises(ValueError):
        eng.bucket_sum_bytes(c["k_words"][:7], c["enc"][:7], 3, 4)


def test_unsynchronised_dev_calls_after_reserve(eng):
    """After bucket_sum_reserve for the larger of the two, two _dev calls of different windows and an msm_dev call on the same context,
    none waited for: all three equal their expectations after one sync."""
    import torch
    c = pool(eng)
    eng.reserve(3 * 257)
    eng.bucket_sum_reserve(3, 257, 8)
    eng.bucket_sum_reserve(3, 257, 5)
    eng.sync()
    n = 3 * 257
    read_a, keep_a = dev_affine(eng, c["k_words"][:n], c["P"][:n], 3, 257, 8, sync=False)
    read_b, keep_b = dev_affine(eng, c["k_words"][:130], c["P"][:130], 2, 65, 5, sync=False)
    out_c = torch.full((5, 64), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    keep_c = (to_dev(c["k_words"][:n]), to_dev(c["P"][:n]))
    eng.msm_dev(keep_c[0], keep_c[1], out_c, 3, 257)
    eng.sync()
    got_c = out_c.cpu().numpy().view(np.uint64)
    assert np.array_equal(read_a()[:3], expected(eng, 3, 257)[0]) and (read_a()[3:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(read_b()[:2], expected(eng, 2, 65)[0]) and (read_b()[2:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(got_c[:3], expected(eng, 3, 257)[0]) and (got_c[3:].view(np.uint8) == 0xA5).all()
