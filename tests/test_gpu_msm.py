"""Grouped multi-scalar multiplication on the device: out[g] = sum_j [k_gj]P_gj (fourq_msm_*, msm_fold_kernel behind the ladder).

Expected values never come from the code under test: the real reference's answers recorded in tests/golden/msm.json, and the group law
sum [k_i][t_i]G = [(sum k_i t_i) mod N]G with the modular arithmetic in Python integers and the point work in the C oracle.
tests/test_msm_oracle.py pins both against each other on the CPU.  Every test takes `eng`, so everything runs with table selection by
address and with constant-time selection; the inputs and expectations are computed once and shared by both.

The fold factor built is 64 and a team is at most 16 lanes wide, so group sizes 63, 64, 65 and 64^2 + 1 = 4097 (all in SIZES) are the ones
at which a second and a third pass start; 3, 5, 31, 33 leave lanes of a team and teams of a wave with nothing but the neutral to add.
Elements handed to the calls under test across this file: 50 333 by the shapes, about 13 200 by the rest, below 2^16 (tests/test_msm_oracle.py
needs none)."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import adversarial_points as adv
import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_scalars
from conftest import ROOT, load_golden
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu

G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
NEUTRAL_AFFINE = codec.pack_points([((0, 0), (1, 0))], 2)[0]
NEUTRAL_ENC = np.frombuffer(bytes([1] + [0] * 31), dtype=np.uint8)
TOP = (1 << 256) - 1
SIZES = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 129, 257, 4097]     # 63, 64, 65, 4097: F - 1, F, F + 1, F^2 + 1 for the fold factor F = 64
GROUPS = [1, 3, 67]
SHAPES = [(g, s) for s in SIZES for g in (GROUPS if s < 257 else [1])]
POOL = 67 * 129                                                       # the largest shape
STATUS = {"Malformed point: reserved bit is not zero": _lib.DECODE_RESERVED_BIT, "Point not on curve": _lib.DECODE_NOT_ON_CURVE,
          "type object 'GFp' has no attribute 'two'": _lib.DECODE_REF_ATTRIBUTE_ERROR}
ROUTE_HOOKS = {"one lane": {"FOURQ_PAIR_MAX": "0"}, "two lanes": {"FOURQ_QUAD_MAX": "0"}, "four lanes": {}}
HOOKS = ("FOURQ_PAIR_MAX", "FOURQ_QUAD_MAX", "FOURQ_FUSED_IO")

_cache = {}


def pool(eng):
    """POOL seeded scalars k and points P_i = [t_i]G from the comb call, checked against the C oracle; a few k are the edge values.
    One per session: both selection modes share it."""
    if "pool" not in _cache:
        table = oc.table(oc.ENDO, G1_WORDS)
        k = codec.unpack_scalars(seeded_scalars(7100, POOL))
        for i, e in enumerate((0, 1, o.N, TOP, o.N - 1, o.N + 1)):
            k[1 + 7 * i] = e
            k[POOL - 1 - 5 * i] = e
        t_words = seeded_scalars(7101, POOL)
        P, st = eng.comb_mul(t_words, eng.comb_table(G1_WORDS))
        assert not st.any()
        assert np.array_equal(P, oc.r1_to_affine(oc.mul(oc.ENDO, t_words, None, table)))
        _cache["pool"] = {"k": k, "t": codec.unpack_scalars(t_words), "k_words": codec.pack_scalars(k), "P": P, "enc": oc.encode(P), "table": table}
    return _cache["pool"]


def group_law(c, index_groups):
    """affine words and encodings of [(sum over i in group of k_i t_i) mod N]G through the C oracle, one row per group of pool indices"""
    sums = [sum(c["k"][i] * c["t"][i] for i in idx) % o.N for idx in index_groups]
    want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, c["table"]))
    return want, oc.encode(want)


def expected(eng, groups, size):
    key = ("want", groups, size)
    if key not in _cache:
        _cache[key] = group_law(pool(eng), [range(g * size, (g + 1) * size) for g in range(groups)])
    return _cache[key]


def mismatches(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def dev_msm(eng, k, P, groups, size):
    import torch
    out = torch.empty((groups, 8), dtype=torch.int64, device=torch.device("cuda", 0))
    eng.msm_dev(to_dev(k), to_dev(P), out, groups, size)
    eng.sync()
    return out.cpu().numpy().view(np.uint64)


def dev_msm_bytes(eng, k, enc, groups, size):
    import torch
    dev = torch.device("cuda", 0)
    out, st = torch.empty((groups, 32), dtype=torch.uint8, device=dev), torch.empty(groups, dtype=torch.uint8, device=dev)
    eng.msm_bytes_dev(to_dev(k), to_dev(enc), out, st, groups, size)
    eng.sync()
    return out.cpu().numpy(), st.cpu().numpy()


def hex_rows(values):
    return np.frombuffer(b"".join(bytes.fromhex("%064x" % v) for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def refused():
    """{FOURQ_DECODE_* code: 32-byte strings} that the reference's decode refuses, by the outcomes recorded in tests/golden/adversarial_points.json:
    the encodings of the fixture's points with an imaginary x, and the strings of tests/adversarial_points.py's two string families"""
    if "refused" not in _cache:
        g = load_golden("adversarial_points.json", raw=True)
        code = lambda outcome: STATUS[g["_outcomes"][int(outcome[1:])][1]]
        out = {}
        for enc, outcome in g["members"]["imaginary_x"]:
            if outcome.startswith("!"):
                out.setdefault(code(outcome), []).append(np.frombuffer(bytes.fromhex(enc), dtype=np.uint8))
        for name, members in (("subfield_y", adv.subfield_y()), ("edge_words_y", adv.edge_words_y())):
            assert len(members) == len(g["members"][name])
            for (_, b), outcome in zip(members, g["members"][name]):
                if outcome.startswith("!"):
                    out.setdefault(code(outcome), []).append(np.frombuffer(b, dtype=np.uint8))
        assert set(out) == {1, 2, 3} and all(len(v) >= 4 for v in out.values())
        _cache["refused"] = out
    return _cache["refused"]


# ---- 1. the reference's own answers, through all four entry points ---------------------------------------------------------------------
def test_fixture_parity_through_all_four_entry_points(eng, golden):
    by_size = {}
    for g in golden("msm.json")["groups"]:
        by_size.setdefault(g["group_size"], []).append(g)
    assert sorted(by_size) == [1, 2, 3, 5, 8]
    for size, gs in by_size.items():
        k = codec.pack_scalars([k for g in gs for k in g["k"]])
        P = codec.pack_points([P for g in gs for P in g["P"]], 2)
        enc = hex_rows(e for g in gs for e in g["P_enc"])
        want, want_enc = codec.pack_points([g["R"] for g in gs], 2), hex_rows(g["R_enc"] for g in gs)
        labels = [g["_label"] for g in gs]
        got = eng.msm(k, P, size)
        assert mismatches(got, want).size == 0, (size, [labels[i] for i in mismatches(got, want)])
        out, st = eng.msm_bytes(k, enc, size)
        assert not st.any() and mismatches(out, want_enc).size == 0, (size, [labels[i] for i in mismatches(out, want_enc)])
        assert mismatches(dev_msm(eng, k, P, len(gs), size), want).size == 0, size
        out, st = dev_msm_bytes(eng, k, enc, len(gs), size)
        assert not st.any() and mismatches(out, want_enc).size == 0, size
    # the neutral point is a result like any other: (0, 1), encoding 01 00 .. 00, no status
    neutral = [g for g in golden("msm.json")["groups"] if g["R"] == ((0, 0), (1, 0))]
    assert len(neutral) >= 3 and all(bytes.fromhex("%064x" % g["R_enc"]) == NEUTRAL_ENC.tobytes() for g in neutral)


# ---- 2. every shape at which the fold takes another path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes_against_the_group_law(eng, groups, size):
    """Teams that do not fill a wave, tail lanes that carry the neutral, a second pass from 65 and a third at 4097.  The affine words at
    every shape; the encoded bytes wherever groups <= 3 (the 67-group shapes of the bytes flavour run in the _dev test below)."""
    c = pool(eng)
    n = groups * size
    want, want_enc = expected(eng, groups, size)
    got = eng.msm(c["k_words"][:n], c["P"][:n], size)
    assert got.shape == (groups, 8) and mismatches(got, want).size == 0, mismatches(got, want)[:8]
    if groups <= 3:
        out, st = eng.msm_bytes(c["k_words"][:n], c["enc"][:n], size)
        assert out.shape == (groups, 32) and not st.any() and mismatches(out, want_enc).size == 0, mismatches(out, want_enc)[:8]


def test_shape_list_is_the_one_promised():
    assert sum(g * s for g, s in SHAPES) + sum(g * s for g, s in SHAPES if g <= 3) == 50333
    assert {63, 64, 65, 64 * 64 + 1} <= set(SIZES) and len(SHAPES) == 12 * 3 + 2


# ---- 3. the order of folding does not show --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,size", [(3, 5), (3, 65), (1, 257)])
def test_permuting_a_group_changes_no_byte(eng, groups, size):
    c = pool(eng)
    n = groups * size
    rng = random.Random(7300 + size)
    idx = np.concatenate([g * size + np.array(rng.sample(range(size), size)) for g in range(groups)])
    assert not np.array_equal(idx, np.arange(n))
    want, want_enc = expected(eng, groups, size)
    assert np.array_equal(eng.msm(c["k_words"][:n][idx], c["P"][:n][idx], size), want)
    out, st = eng.msm_bytes(c["k_words"][:n][idx], c["enc"][:n][idx], size)
    assert not st.any() and np.array_equal(out, want_enc)


# ---- 4. ragged groups, padded -----------------------------------------------------------------------------------------------------------
def test_ragged_groups_padded_with_scalar_zero(eng):
    """Groups of 1 .. 65 elements padded to 65 with scalar 0 equal the unpadded sums (group law).  Affine flavour: the pad point is the
    neutral (0, 1).  Bytes flavour: the pad is any string that decodes, here encode(G) -- the neutral's own encoding 01 00 .. 00 is one the
    reference's decode refuses (FOURQ_DECODE_REF_ATTRIBUTE_ERROR), so a group padded with it reports that and is zeroed."""
    c = pool(eng)
    lengths, size = [1, 3, 64, 65, 2, 33, 17], 65
    starts = np.cumsum([0] + lengths[:-1])
    want, want_enc = group_law(c, [range(s, s + n) for s, n in zip(starts, lengths)])
    k = np.zeros((len(lengths) * size, 4), dtype=np.uint64)
    P = np.tile(NEUTRAL_AFFINE, (len(lengths) * size, 1))
    enc = np.tile(oc.encode(codec.pack_points([(o.Gx, o.Gy)], 2))[0], (len(lengths) * size, 1))
    enc_neutral = np.tile(NEUTRAL_ENC, (len(lengths) * size, 1))
    for g, (s, n) in enumerate(zip(starts, lengths)):
        k[g * size:g * size + n], P[g * size:g * size + n] = c["k_words"][s:s + n], c["P"][s:s + n]
        enc[g * size:g * size + n] = enc_neutral[g * size:g * size + n] = c["enc"][s:s + n]
    assert np.array_equal(eng.msm(k, P, size), want)
    out, st = eng.msm_bytes(k, enc, size)
    assert not st.any() and np.array_equal(out, want_enc)
    out, st = eng.msm_bytes(k, enc_neutral, size)
    padded = np.array([n < size for n in lengths])
    assert np.array_equal(st, np.where(padded, _lib.BYTES_DECODE_BASE + _lib.DECODE_REF_ATTRIBUTE_ERROR, 0).astype(np.uint8))
    assert not out[padded].any() and np.array_equal(out[~padded], want_enc[~padded])


# ---- 5. encodings that do not decode ---------------------------------------------------------------------------------------------------
def test_undecodable_elements_mark_their_group_only(eng):
    """5 groups of 129 (two passes: 129 -> 3 -> 1 rows, teams of 16 and of 4 lanes).  Bad strings at the first position, at the last (the
    one-row third segment), two codes in one group in different segments and lanes (30 and 100), and two in ONE lane's rows (5 and
    21); group 4 stays clean.  status[g] = 16 + the larger code, out32[g] zero, every other group exact."""
    c = pool(eng)
    bad = refused()
    groups, size = 5, 129
    n = groups * size
    want, want_enc = expected(eng, groups, size)
    enc = c["enc"][:n].copy()
    plan = {0: [(0, 2)], 1: [(128, 1)], 2: [(30, 3), (100, 1)], 3: [(5, 1), (21, 2)]}
    want_st = np.zeros(groups, dtype=np.uint8)
    for g, cells in plan.items():
        for j, (pos, code) in enumerate(cells):
            enc[g * size + pos] = bad[code][(g + j) % len(bad[code])]
        want_st[g] = _lib.BYTES_DECODE_BASE + max(code for _, code in cells)
    assert list(want_st) == [18, 17, 19, 18, 0]
    for out, st in (eng.msm_bytes(c["k_words"][:n], enc, size), dev_msm_bytes(eng, c["k_words"][:n], enc, groups, size)):
        assert np.array_equal(st, want_st)
        assert not out[:4].any() and np.array_equal(out[4], want_enc[4])
    # each bad group among good ones, in a small shape too: 3 groups of 3, the middle one spoiled at its last element
    want3, want3_enc = expected(eng, 3, 3)
    enc = c["enc"][:9].copy()
    enc[5] = bad[3][0]
    out, st = eng.msm_bytes(c["k_words"][:9], enc, 3)
    assert list(st) == [0, 19, 0] and not out[1].any() and np.array_equal(out[[0, 2]], want3_enc[[0, 2]])


# ---- 6. every route of the ladder in front: rows of 12 words and of 20 --------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTE_HOOKS))
def test_every_ladder_route(eng, route, monkeypatch):
    from fourq_amd import Engine
    for key in HOOKS:
        monkeypatch.delenv(key, raising=False)
    for key, value in ROUTE_HOOKS[route].items():
        monkeypatch.setenv(key, value)
    c = pool(eng)
    groups, size = 3, 65
    n = groups * size
    want, want_enc = expected(eng, groups, size)
    enc = c["enc"][:n].copy()
    enc[size + 64] = refused()[2][1]
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        assert np.array_equal(e.msm(c["k_words"][:n], c["P"][:n], size), want)
        out, st = e.msm_bytes(c["k_words"][:n], enc, size)
        assert list(st) == [0, 18, 0] and not out[1].any() and np.array_equal(out[[0, 2]], want_enc[[0, 2]])


# ---- 7. the _dev flavour and the argument rules ---------------------------------------------------------------------------------------------
def test_dev_flavour_after_reserve_and_argument_rules(eng):
    import torch
    c = pool(eng)
    eng.reserve(67 * 65)
    for groups, size in ((3, 257), (67, 33), (67, 65)):
        n = groups * size
        want, want_enc = expected(eng, groups, size)
        if groups == 3:
            assert np.array_equal(dev_msm(eng, c["k_words"][:n], c["P"][:n], groups, size), want)
            assert np.array_equal(eng.msm(c["k_words"][:n], c["P"][:n], size), want)
        else:
            out, st = dev_msm_bytes(eng, c["k_words"][:n], c["enc"][:n], groups, size)
            assert not st.any() and np.array_equal(out, want_enc), (groups, size)
    lib, ctx, dev = eng._lib, eng._ctx, torch.device("cuda", 0)
    k, P, enc = to_dev(c["k_words"][:16]), to_dev(c["P"][:16]), to_dev(c["enc"][:16])
    out = torch.full((5, 8), -1, dtype=torch.int64, device=dev)
    out32, st = torch.empty((4, 32), dtype=torch.uint8, device=dev), torch.empty(4 + 1, dtype=torch.uint8, device=dev)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    affine, bytes_ = lib.fourq_msm_affine_batch_dev, lib.fourq_msm_bytes_batch_dev
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 4, 4) == _lib.OK
    # every array pointer 16-byte aligned; status need not be
    assert affine(ctx, ptr(k, 8), ptr(P), ptr(out), 3, 4) == _lib.ERR_INVALID
    assert affine(ctx, ptr(k), ptr(P, 8), ptr(out), 3, 4) == _lib.ERR_INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out, 8), 3, 4) == _lib.ERR_INVALID
    assert bytes_(ctx, ptr(k), ptr(enc, 8), ptr(out32), ptr(st), 3, 4) == _lib.ERR_INVALID
    assert bytes_(ctx, ptr(k), ptr(enc), ptr(out32), ptr(st, 1), 4, 4) == _lib.OK
    eng.sync()
    want4, want4_enc = group_law(c, [range(g * 4, g * 4 + 4) for g in range(4)])
    assert np.array_equal(out.cpu().numpy().view(np.uint64)[:4], want4) and (out.cpu().numpy()[4] == -1).all()
    assert np.array_equal(out32.cpu().numpy(), want4_enc) and not st.cpu().numpy()[1:].any()
    # the count: group_size 0, a product above FOURQ_MAX_BATCH, one that overflows size_t; no groups is no work
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 4, 0) == _lib.ERR_INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 1 << 16, 1 << 16) == _lib.ERR_INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out), _lib.MAX_BATCH // 2 + 1, 2) == _lib.ERR_INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 1 << 63, 2) == _lib.ERR_INVALID
    assert bytes_(ctx, ptr(k), ptr(enc), ptr(out32), ptr(st), (1 << 62) + 1, 4) == _lib.ERR_INVALID
    assert affine(ctx, ptr(k), ptr(P), ptr(out), 0, 4) == _lib.OK and affine(ctx, ptr(k), ptr(P), ptr(out), 0, 0) == _lib.OK
    assert lib.fourq_msm_affine_batch(ctx, None, None, None, 0, 0) == _lib.ERR_INVALID
    host_out = np.full((2, 8), 7, dtype=np.uint64)
    assert lib.fourq_msm_affine_batch(ctx, c["k_words"].ctypes.data, c["P"].ctypes.data, host_out.ctypes.data, 0, 3) == _lib.OK and (host_out == 7).all()
    assert lib.fourq_msm_affine_batch(ctx, c["k_words"].ctypes.data, c["P"].ctypes.data, host_out.ctypes.data, 2, 0) == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        eng.msm(c["k_words"][:7], c["P"][:7], 2)
    with pytest.raises(ValueError):
        eng.msm_bytes(c["k_words"][:7], c["enc"][:7], 3)


# ---- 8. the C ABI from C ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_c_host_program_checks_fixture_groups(eng, golden, tmp_path):
    from fourq_amd.build import LIB_PATH
    gs = [g for g in golden("msm.json")["groups"] if g["group_size"] == 8]
    assert len(gs) >= 3
    src = os.path.join(ROOT, "tests", "c", "msm_check.c")
    exe, libdir = str(tmp_path / "msm_check"), os.path.dirname(LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                    "-L", libdir, "-lfourq_amd", "-Wl,-rpath," + libdir], check=True)
    path = tmp_path / "vectors.bin"
    with open(path, "wb") as fh:
        for v in (len(gs), 8, 1 if eng.ct_select else 0):
            fh.write(np.uint64(v).tobytes())
        for a in (codec.pack_scalars([k for g in gs for k in g["k"]]), codec.pack_points([P for g in gs for P in g["P"]], 2),
                  codec.pack_points([g["R"] for g in gs], 2)):
            fh.write(np.ascontiguousarray(a, dtype="<u8").tobytes())
        fh.write(hex_rows(e for g in gs for e in g["P_enc"]).tobytes())
        fh.write(hex_rows(g["R_enc"] for g in gs).tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")     # no PyTorch in a C program: the system HIP runtime
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "grouped sums bit-exact through the C ABI" in proc.stdout
