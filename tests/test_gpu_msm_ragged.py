"""Ragged grouped sums on the device: out[g] = sum over group g of [k_i]P_i over groups of any length, 0 included (fourq_raggedsum_*,
msm_fold_desc_kernel behind the ladder, the passes planned on the host by fourq_amd/csrc/msm_shape.h).

Expected values never come from the code under test: the group law sum [k_i][t_i]G = [(sum k_i t_i) mod N]G with the modular arithmetic
in Python integers and the point work in the C oracle, over the pool of points tests/test_gpu_msm.py builds (one per session, shared);
decode statuses from the outcomes recorded in tests/golden/adversarial_points.json.  tests/test_msm_ragged_oracle.py pins the planner on
the CPU.  Every test takes `eng`, so everything runs with table selection by address and with constant-time selection.

The fold factor is 64 and a team is at most 16 lanes wide.  The shapes (lengths per group):
  A   empties first, last, in the middle and adjacent; 63, 64, 65 next to each other; two passes for some groups while others are at one row
  B   64^2 + 1 rows: three passes for one group, its neighbours (one empty) ride through them as single rows
  C   67 groups of one row: no pass at all
  D   five empty groups: no row, no ladder launch, five neutrals
  E   widths below 16 leave lanes idle
  Eq  equal lengths: the bytes of fourq_msm_*
Ladder rows handed to the calls under test per selection mode: about 22 000."""
import ctypes

import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
from fourq_amd import FourQError, _lib, codec
from test_gpu_msm import NEUTRAL_AFFINE, NEUTRAL_ENC, TOP, mismatches, pool, refused, to_dev

pytestmark = pytest.mark.gpu

A = [0, 1, 0, 0, 2, 63, 64, 65, 0, 127, 129, 1, 0]
B = [4097, 0, 1]
C = [1] * 67
D = [0] * 5
E = [3, 5, 31, 33, 17]
EQ = [65] * 3
SHAPES = {"A": A, "B": B, "C": C, "D": D, "E": E}
_cache = {}


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)


def case(eng, spec):
    """spec: per group a list of (scalar, pool index).  The arrays the calls take, the offsets, and what the group law says comes out:
    [(sum k_i t_i) mod N]G per group through the C oracle -- the neutral, (0, 1) and 01 00 .. 00, for an empty group."""
    c = pool(eng)
    ks = [k for g in spec for k, _ in g]
    idx = np.array([i for g in spec for _, i in g], dtype=np.int64)
    sums = [sum(k * c["t"][i] for k, i in g) % o.N for g in spec]
    want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, c["table"]))
    want_enc = oc.encode(want)
    for g, rows in enumerate(spec):
        if not rows:
            assert np.array_equal(want[g], NEUTRAL_AFFINE) and np.array_equal(want_enc[g], NEUTRAL_ENC)
    k_words = codec.pack_scalars(ks) if ks else np.zeros((0, 4), dtype=np.uint64)
    return {"k": k_words, "P": c["P"][idx], "enc": c["enc"][idx], "offsets": offsets_of([len(g) for g in spec]), "want": want, "want_enc": want_enc,
            "groups": len(spec), "n": len(ks)}


def shape_case(eng, name, lengths):
    """the pool's first rows, scalars and points as they lie, cut into groups of these lengths; computed once and shared by both modes"""
    if name not in _cache:
        c = pool(eng)
        starts = np.concatenate([[0], np.cumsum(lengths)])
        _cache[name] = case(eng, [[(c["k"][i], i) for i in range(s, s + n)] for s, n in zip(starts, lengths)])
    return _cache[name]


def dev_rows(a, cols, dtype):
    """a device tensor of the rows; one spare row where there is none, so that the pointer is a real, aligned one"""
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1, cols)
    return to_dev(a if len(a) else np.zeros((1, cols), dtype=dtype))


def dev_ragged(eng, k, P, groups):
    import torch
    out = torch.full((groups + 1, 8), -1, dtype=torch.int64, device=torch.device("cuda", 0))
    eng.msm_ragged_dev(dev_rows(k, 4, np.uint64), dev_rows(P, 8, np.uint64), out)
    eng.sync()
    got = out.cpu().numpy()
    assert (got[groups] == -1).all()                            # nothing behind the last group's row
    return got[:groups].view(np.uint64)


def dev_ragged_bytes(eng, k, enc, groups):
    import torch
    dev = torch.device("cuda", 0)
    out, st = torch.full((groups + 1, 32), 0xA5, dtype=torch.uint8, device=dev), torch.full((groups + 1,), 0xA5, dtype=torch.uint8, device=dev)
    eng.msm_ragged_bytes_dev(dev_rows(k, 4, np.uint64), dev_rows(enc, 32, np.uint8), out, st)
    eng.sync()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert (out[groups] == 0xA5).all() and st[groups] == 0xA5
    return out[:groups], st[:groups]


# ---- 4. values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_group_law(eng, name):
    """Both flavours, host arrays and _dev, on every shape; on B (4 098 rows) the affine flavour through host arrays and the bytes flavour
    through _dev."""
    lengths = SHAPES[name]
    s = shape_case(eng, name, lengths)
    groups = len(lengths)
    empty = np.array([n == 0 for n in lengths])
    assert np.array_equal(s["want"][empty], np.tile(NEUTRAL_AFFINE, (empty.sum(), 1)))
    got = eng.msm_ragged(s["k"], s["P"], s["offsets"])
    assert eng.msm_shape_count() == (groups, sum(lengths))
    assert got.shape == (groups, 8) and mismatches(got, s["want"]).size == 0, mismatches(got, s["want"])[:8]
    out, st = dev_ragged_bytes(eng, s["k"], s["enc"], groups)
    assert not st.any() and mismatches(out, s["want_enc"]).size == 0, mismatches(out, s["want_enc"])[:8]
    assert np.array_equal(out[empty], np.tile(NEUTRAL_ENC, (empty.sum(), 1)))
    if name != "B":
        assert mismatches(dev_ragged(eng, s["k"], s["P"], groups), s["want"]).size == 0
        out, st = eng.msm_ragged_bytes(s["k"], s["enc"])                # offsets=None: the installed shape
        assert out.shape == (groups, 32) and st.shape == (groups,) and not st.any() and mismatches(out, s["want_enc"]).size == 0


# ---- 5. identity with the equal-length call ---------------------------------------------------------------------------------------------
def test_equal_lengths_give_the_bytes_of_the_grouped_call(eng):
    s = shape_case(eng, "Eq", EQ)
    assert np.array_equal(s["want"], eng.msm(s["k"], s["P"], 65))
    got = eng.msm_ragged(s["k"], s["P"], s["offsets"])
    assert np.array_equal(got, s["want"]) and np.array_equal(got, eng.msm(s["k"], s["P"], 65))
    out, st = eng.msm_ragged_bytes(s["k"], s["enc"], s["offsets"])
    out65, st65 = eng.msm_bytes(s["k"], s["enc"], 65)
    assert np.array_equal(out, out65) and np.array_equal(st, st65) and np.array_equal(out, s["want_enc"]) and not st.any()


def test_each_group_equals_the_grouped_call_over_that_group_alone(eng):
    s = shape_case(eng, "A", A)
    got = eng.msm_ragged(s["k"], s["P"], s["offsets"])
    out, st = eng.msm_ragged_bytes(s["k"], s["enc"])
    for g, n in enumerate(A):
        lo = int(s["offsets"][g])
        if n:
            assert np.array_equal(got[g:g + 1], eng.msm(s["k"][lo:lo + n], s["P"][lo:lo + n], n)), g
            alone, alone_st = eng.msm_bytes(s["k"][lo:lo + n], s["enc"][lo:lo + n], n)
            assert np.array_equal(out[g:g + 1], alone) and st[g] == alone_st[0] == 0, g


# ---- 6. scalars at the edges ------------------------------------------------------------------------------------------------------------
def test_edge_scalars_at_the_ends_of_groups_zero_groups_and_cancelling_terms(eng):
    """0, 1, N - 1, N, N + 1, 2^256 - 1 each at the first row of one group and at the last row of another, in groups of 3, 4, 65, 64, 5 and
    66 rows; an empty group; a group whose scalars are all zero; and one whose two terms k, N - k on one point cancel: both give the neutral
    from non-empty input."""
    c = pool(eng)
    edges = [0, 1, o.N - 1, o.N, o.N + 1, TOP]
    spec, at = [], 100
    for i, n in enumerate([3, 4, 65, 64, 5, 66]):
        rows = [(c["k"][j], j) for j in range(at, at + n)]
        rows[0], rows[-1] = (edges[i], at), (edges[(i + 3) % 6], at + n - 1)
        spec.append(rows)
        at += n
    spec.insert(3, [])
    spec.append([(0, j) for j in range(at, at + 4)])
    k = c["k"][at + 9] % o.N or 5
    spec.append([(k, at + 10), (o.N - k, at + 10)])
    s = case(eng, spec)
    neutral = [3, len(spec) - 2, len(spec) - 1]
    assert np.array_equal(s["want"][neutral], np.tile(NEUTRAL_AFFINE, (3, 1))) and (s["want"][[0, 1, 2, 4, 5, 6]] != NEUTRAL_AFFINE).any(axis=1).all()
    got = eng.msm_ragged(s["k"], s["P"], s["offsets"])
    assert mismatches(got, s["want"]).size == 0, mismatches(got, s["want"])
    out, st = eng.msm_ragged_bytes(s["k"], s["enc"])
    assert not st.any() and mismatches(out, s["want_enc"]).size == 0, mismatches(out, s["want_enc"])
    assert np.array_equal(out[neutral], np.tile(NEUTRAL_ENC, (3, 1)))
    assert mismatches(dev_ragged(eng, s["k"], s["P"], s["groups"]), s["want"]).size == 0


# ---- 7. encodings that do not decode ------------------------------------------------------------------------------------------------------
def test_undecodable_rows_mark_their_group_only(eng):
    """Shape A, bytes.  One refused string of each recorded class, one by one, at the first row of a group (the 63 rows of group 5), at the
    last row (group 9, 127 rows: the last lane's last row of the second segment) and at a row past position 64 (row 100 of group 10): that
    group reports 16 + the code and a zero row; every other group -- the empty neighbours 8 and 12 included -- is what the clean run gives.
    Then two classes in one group, in different segments, and a third in the one-row second segment of the 65-row group: the larger code."""
    s = shape_case(eng, "A", A)
    bad = refused()
    assert sorted(bad) == [_lib.DECODE_RESERVED_BIT, _lib.DECODE_NOT_ON_CURVE, _lib.DECODE_REF_ATTRIBUTE_ERROR]
    eng.msm_shape(s["offsets"])
    clean, clean_st = eng.msm_ragged_bytes(s["k"], s["enc"])
    assert not clean_st.any() and np.array_equal(clean, s["want_enc"])
    cells = [(5, 0), (9, A[9] - 1), (10, 100)]
    for code in sorted(bad):
        for which, (g, pos) in enumerate(cells):
            enc = s["enc"].copy()
            enc[int(s["offsets"][g]) + pos] = bad[code][which % len(bad[code])]
            call = eng.msm_ragged_bytes if which != 1 else (lambda k, e: dev_ragged_bytes(eng, k, e, len(A)))
            out, st = call(s["k"], enc)
            others = np.arange(len(A)) != g
            assert st[g] == _lib.BYTES_DECODE_BASE + code and not out[g].any(), (code, g, pos)
            assert not st[others].any() and np.array_equal(out[others], s["want_enc"][others]), (code, g, pos)
    enc = s["enc"].copy()
    enc[int(s["offsets"][10]) + 3], enc[int(s["offsets"][10]) + 70] = bad[1][0], bad[3][1]
    enc[int(s["offsets"][7]) + 64] = bad[2][2]
    out, st = eng.msm_ragged_bytes(s["k"], enc)
    spoiled = np.isin(np.arange(len(A)), [7, 10])
    assert st[10] == 19 and st[7] == 18 and not out[spoiled].any()
    assert not st[~spoiled].any() and np.array_equal(out[~spoiled], s["want_enc"][~spoiled])


# ---- 8. the shape's lifecycle -------------------------------------------------------------------------------------------------------------
def test_shape_lifecycle(eng):
    import torch
    from fourq_amd import Engine
    a, e_ = shape_case(eng, "A", A), shape_case(eng, "E", E)
    c = pool(eng)
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        # no shape yet
        assert e.msm_shape_count() == (0, 0)
        with pytest.raises(FourQError):
            e.msm_ragged(a["k"], a["P"])
        with pytest.raises(FourQError):
            e.msm_shape_reserve()
        lib, ctx = e._lib, e._ctx
        assert lib.fourq_raggedsum_affine(ctx, a["k"].ctypes.data, a["P"].ctypes.data, np.zeros((13, 8), dtype=np.uint64).ctypes.data) == _lib.ERR_INVALID
        e.msm_shape(a["offsets"])
        assert e.msm_shape_count() == (len(A), sum(A))
        # an invalid shape is refused and the old one goes on working
        offs = lambda *v: np.array(v, dtype=np.uint32)
        for bad in (offs(0, 5, 4, 9), offs(1, 2, 3), offs(0), offs(0, 0xffffff01)):
            assert lib.fourq_raggedsum_shape_set(ctx, bad.ctypes.data, len(bad) - 1) == _lib.ERR_INVALID
            with pytest.raises((FourQError, ValueError)):
                e.msm_shape(bad)
        assert lib.fourq_raggedsum_shape_set(ctx, None, 3) == _lib.ERR_INVALID and lib.fourq_raggedsum_shape_set(None, a["offsets"].ctypes.data, 13) == _lib.ERR_INVALID
        groups, rows = ctypes.c_size_t(7), ctypes.c_size_t(7)
        assert lib.fourq_raggedsum_shape_count(None, ctypes.byref(groups), ctypes.byref(rows)) == _lib.ERR_INVALID and lib.fourq_raggedsum_shape_reserve(None) == _lib.ERR_INVALID
        assert e.msm_shape_count() == (len(A), sum(A))
        assert np.array_equal(e.msm_ragged(a["k"], a["P"]), a["want"])
        # other state of the context set between shape_set and the call changes nothing, and the shape survives a change of stream
        e.commit_bases(c["P"][:3])
        e.keyset_set(c["enc"][:4])
        e.comb_stage(e.comb_table(codec.pack_point(o.AffineToR1(o.Gx, o.Gy))))
        side = torch.cuda.Stream(device=torch.device("cuda", 0))
        e.set_stream(side.cuda_stream)
        try:
            assert e.msm_shape_count() == (len(A), sum(A))
            out, st = e.msm_ragged_bytes(a["k"], a["enc"])
            assert not st.any() and np.array_equal(out, a["want_enc"])
        finally:
            e.set_stream(None)
        assert e.commit_bases_count == 3 and e.keyset_count() == 4
        # A replaced by E
        assert np.array_equal(e.msm_ragged(e_["k"], e_["P"], e_["offsets"]), e_["want"])
        assert e.msm_shape_count() == (len(E), sum(E))
        out, st = e.msm_ragged_bytes(e_["k"], e_["enc"])
        assert not st.any() and np.array_equal(out, e_["want_enc"])
        # wrong array lengths
        with pytest.raises(ValueError):
            e.msm_ragged(a["k"], a["P"])
        with pytest.raises(ValueError):
            e.msm_ragged(e_["k"], e_["P"][:-1])
        with pytest.raises(ValueError):
            e.msm_ragged_bytes(e_["k"][:-1], e_["enc"][:-1], e_["offsets"])
        with pytest.raises(ValueError):
            e.msm_ragged(e_["k"], e_["P"], a["offsets"])
        with pytest.raises(ValueError):
            e.msm_ragged(e_["k"], e_["P"], e_["offsets"], out=np.zeros((len(E) + 1, 8), dtype=np.uint64))
        e.msm_shape(e_["offsets"])
        assert np.array_equal(e.msm_ragged(e_["k"], e_["P"]), e_["want"])


# ---- 9. after reserve a _dev call only enqueues ---------------------------------------------------------------------------------------------
def test_dev_call_after_reserve_is_captured_into_a_graph_and_back_to_back_calls_agree(eng):
    """A stream capture takes no allocation and no synchronisation: after msm_shape_reserve the call is captured as it stands, and the replay
    over other inputs gives their sums.  Then two _dev calls back to back without a synchronisation between them against the same two
    synchronised: the second reuses the work buffer behind the first in stream order."""
    import torch
    dev = torch.device("cuda", 0)
    s = shape_case(eng, "A", A)
    groups, n = len(A), sum(A)
    # a second set of inputs on the same shape: the pool's rows from 1000 on
    c = pool(eng)
    starts = np.concatenate([[0], np.cumsum(A)]) + 1000
    s2 = case(eng, [[(c["k"][i], i) for i in range(lo, lo + m)] for lo, m in zip(starts, A)])
    eng.msm_shape(s["offsets"])
    d_k, d_enc = to_dev(s["k"]), to_dev(s["enc"])
    out, st = torch.empty((groups, 32), dtype=torch.uint8, device=dev), torch.empty(groups, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    try:
        eng.msm_shape_reserve()
        eng.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            eng.msm_ragged_bytes_dev(d_k, d_enc, out, st)
            graph.capture_end()
        out.fill_(0xA5)
        st.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), s["want_enc"])
        d_k.copy_(to_dev(s2["k"])); d_enc.copy_(to_dev(s2["enc"]))
        graph.replay()
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), s2["want_enc"])
    finally:
        eng.set_stream(None)
    k1, P1, k2, P2 = to_dev(s["k"]), to_dev(s["P"]), to_dev(s2["k"]), to_dev(s2["P"])
    o1, o2 = (torch.empty((groups, 8), dtype=torch.int64, device=dev) for _ in range(2))
    eng.msm_ragged_dev(k1, P1, o1)
    eng.msm_ragged_dev(k2, P2, o2)
    eng.sync()
    back_to_back = o1.cpu().numpy().view(np.uint64), o2.cpu().numpy().view(np.uint64)
    assert np.array_equal(dev_ragged(eng, s["k"], s["P"], groups), back_to_back[0]) and np.array_equal(dev_ragged(eng, s2["k"], s2["P"], groups), back_to_back[1])
    assert np.array_equal(back_to_back[0], s["want"]) and np.array_equal(back_to_back[1], s2["want"])


# ---- 10. the argument contract --------------------------------------------------------------------------------------------------------------
def test_argument_contract_of_the_dev_calls(eng):
    import torch
    s = shape_case(eng, "E", E)
    eng.msm_shape(s["offsets"])
    lib, ctx, dev = eng._lib, eng._ctx, torch.device("cuda", 0)
    k, P, enc = to_dev(s["k"]), to_dev(s["P"]), to_dev(s["enc"])
    out = torch.empty((len(E) + 1, 8), dtype=torch.int64, device=dev)
    out32, st = torch.empty((len(E) + 1, 32), dtype=torch.uint8, device=dev), torch.empty(len(E) + 1, dtype=torch.uint8, device=dev)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    affine, bytes_ = lib.fourq_raggedsum_affine_dev, lib.fourq_raggedsum_bytes_dev
    # a NULL context is refused before anything else is looked at: every other argument is valid
    assert affine(None, ptr(k), ptr(P), ptr(out)) == _lib.ERR_INVALID and bytes_(None, ptr(k), ptr(enc), ptr(out32), ptr(st)) == _lib.ERR_INVALID
    assert lib.fourq_raggedsum_affine(None, s["k"].ctypes.data, s["P"].ctypes.data, np.zeros((5, 8), dtype=np.uint64).ctypes.data) == _lib.ERR_INVALID
    for args in ((None, ptr(P), ptr(out)), (ptr(k), None, ptr(out)), (ptr(k), ptr(P), None), (ptr(k, 8), ptr(P), ptr(out)), (ptr(k), ptr(P, 8), ptr(out)),
                 (ptr(k), ptr(P), ptr(out, 8))):
        assert affine(ctx, *args) == _lib.ERR_INVALID
    for args in ((None, ptr(enc), ptr(out32), ptr(st)), (ptr(k), None, ptr(out32), ptr(st)), (ptr(k), ptr(enc), None, ptr(st)), (ptr(k), ptr(enc), ptr(out32), None),
                 (ptr(k, 8), ptr(enc), ptr(out32), ptr(st)), (ptr(k), ptr(enc, 8), ptr(out32), ptr(st)), (ptr(k), ptr(enc), ptr(out32, 8), ptr(st))):
        assert bytes_(ctx, *args) == _lib.ERR_INVALID
    # the status pointer need not be aligned
    assert affine(ctx, ptr(k), ptr(P), ptr(out)) == _lib.OK and bytes_(ctx, ptr(k), ptr(enc), ptr(out32), ptr(st, 1)) == _lib.OK
    eng.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint64)[:len(E)], s["want"])
    assert np.array_equal(out32.cpu().numpy()[:len(E)], s["want_enc"]) and not st.cpu().numpy()[1:].any()


# ---- 11. the reference's own answers on one ragged shape --------------------------------------------------------------------------------------
def test_fixture_parity_through_all_four_entry_points(eng, golden):
    from test_gpu_msm import hex_rows
    fx = golden("msm_ragged.json")
    gs = fx["groups"]
    lengths = [g["length"] for g in gs]
    assert lengths.count(0) == 4 and max(lengths) > 64
    k = codec.pack_scalars([k for g in gs for k in g["k"]])
    P = codec.pack_points([P for g in gs for P in g["P"]], 2)
    enc = hex_rows(e for g in gs for e in g["P_enc"])
    want, want_enc = codec.pack_points([g["R"] for g in gs], 2), hex_rows(g["R_enc"] for g in gs)
    offsets = offsets_of(lengths)
    got = eng.msm_ragged(k, P, offsets)
    assert mismatches(got, want).size == 0, mismatches(got, want)
    out, st = eng.msm_ragged_bytes(k, enc, offsets)
    assert not st.any() and mismatches(out, want_enc).size == 0, mismatches(out, want_enc)
    assert mismatches(dev_ragged(eng, k, P, len(gs)), want).size == 0
    out, st = dev_ragged_bytes(eng, k, enc, len(gs))
    assert not st.any() and mismatches(out, want_enc).size == 0
