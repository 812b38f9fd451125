"""Commitments over a fixed generator set on the device (fourq_commit_*, fourq_amd/csrc/commit.hip.h): out[g] = sum_j [k_gj]B_j through one
comb per generator, byte for byte what fourq_msm_* gives over the tiled bases.

Expected values never come from the code under test: the bases are B_j = [t_j]G with known t_j (made with the comb call and checked against
the C oracle), so the group law gives out[g] = [(sum_j k_gj t_j) mod N]G, with the sum in Python integers and the point from the C oracle.
tests/test_commit_oracle.py pins the restatement, the fixture and the launch geometry on the CPU -- among it, that 67 x 130 makes blocks
change base inside their item range on a 256-CU chip in both selection modes.  Every test takes `eng`: selection by address runs the staged
and the gather kernel as `route` says, constant-time selection the scan kernel whatever the route; same expectations.

Rows handed to the calls under test across this file, per selection mode: about 110 000 (the shapes 104 000, the rest under 6 000), and one
call of 16 900 (default mode) or 67 600 (constant-time mode) for the smallest shape at which a 256-CU chip gets blocks wider than a wave."""
import ctypes

import numpy as np
import pytest

import bucket_ref
import commit_ref as ref
import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_scalars
from conftest import load_golden
from fourq_amd import Engine, MultiEngine, _lib, codec

pytestmark = pytest.mark.gpu

G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
NEUTRAL_AFFINE = codec.pack_points([((0, 0), (1, 0))], 2)[0]
NEUTRAL_ENC = np.frombuffer(bytes([1] + [0] * 31), dtype=np.uint8)
BASES = 130
SIZES = [1, 2, 3, 63, 64, 65, 130]
EDGES = [(1025, 2), (1025, 3), (2049, 1)]                              # one group past 1 024 lanes of a base; a third slice
SHAPES = [(g, s) for s in SIZES for g in (1, 3, 67)] + EDGES
ROUTES = [1, 2, 0]
WIDE = {False: (130, 130), True: (520, 130)}                           # per selection mode: blocks of two waves that change base in mid-range
POOL = 520 * 130                                                       # the largest shape
P127 = (1 << 127) - 1

_cache = {}


def pool(eng):
    """The 130 bases B_j = [t_j]G from the comb call, checked against the C oracle, and POOL seeded scalars with the six edge values planted
    (bucket_ref.pool_scalars: odd and even ones, the comb negates for even ones).  One per session: both selection modes share it."""
    if "pool" not in _cache:
        table = oc.table(oc.ENDO, G1_WORDS)
        t_words = seeded_scalars(7501, BASES)
        B, st = eng.comb_mul(t_words, eng.comb_table(G1_WORDS))
        assert not st.any()
        assert np.array_equal(B, oc.r1_to_affine(oc.mul(oc.ENDO, t_words, None, table)))
        k = bucket_ref.pool_scalars(POOL, seed=7500)
        assert set(bucket_ref.EDGE_SCALARS) <= set(k[:64]) and k[1] == 0 and k[8] == 1                # even and odd ones from the first rows on
        _cache["pool"] = {"k": k, "k_words": codec.pack_scalars(k), "t": [t % o.N for t in codec.unpack_scalars(t_words)], "B": B, "table": table}
    return _cache["pool"]


def use_set(eng, name, points):
    """make `points` the context's generator set unless the set called `name` is already there"""
    if _cache.get(("set", id(eng))) != name:
        eng.commit_bases(points)
        _cache["set", id(eng)] = name


def main_set(eng):
    c = pool(eng)
    use_set(eng, "main", c["B"])
    assert eng.commit_bases_count == BASES
    return c


def multiples_of_g(c, sums):
    """affine words and encodings of [s mod N]G through the C oracle"""
    want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars([s % o.N for s in sums]), None, c["table"]))
    return want, oc.encode(want)


def expected(eng, groups, size):
    key = ("want", groups, size)
    if key not in _cache:
        c = pool(eng)
        _cache[key] = multiples_of_g(c, [sum(c["k"][g * size + j] * c["t"][j] for j in range(size)) for g in range(groups)])
    return _cache[key]


def mismatches(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def dev_call(eng, k, groups, size, route, encoded=False, sync=True):
    """_dev call into a 0xA5-filled tensor two rows longer than needed: the rows, once synchronised and with the guard rows checked"""
    import torch
    width = 32 if encoded else 64
    out = torch.full((groups + 2, width), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    keep = to_dev(k)
    (eng.commit_bytes_dev if encoded else eng.commit_dev)(keep, out, groups, size, route)

    def read():
        got = out.cpu().numpy()
        assert (got[groups:] == 0xA5).all()
        return got[:groups] if encoded else got[:groups].view(np.uint64)
    if not sync:
        return read, keep
    eng.sync()
    return read()


def check(got, want):
    assert got.shape == want.shape and mismatches(got, want).size == 0, mismatches(got, want)[:8]


# ---- 1. every shape on every route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES, ids=["staged", "gather", "picked"])
@pytest.mark.parametrize("groups,size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes(eng, groups, size, route):
    """Up to three groups: affine and bytes, host arrays and _dev, on every route.  The 67-group shapes and the staged-route edges run one
    flavour per route -- bytes through _dev staged, affine on the host arrays gather, affine through _dev on the library's pick."""
    c = main_set(eng)
    k = c["k_words"][:groups * size]
    want, want_enc = expected(eng, groups, size)
    small = groups <= 3
    if small or route == 2:
        check(eng.commit(k, size, route), want)
    if small or route == 1:
        check(dev_call(eng, k, groups, size, route, encoded=True), want_enc)
    if small or route == 0:
        check(dev_call(eng, k, groups, size, route), want)
    if small:
        check(eng.commit_bytes(k, size, route), want_enc)


def test_shape_list_is_the_one_promised():
    assert set(SIZES) == {1, 2, 3, 63, 64, 65, 130} and set(EDGES) == {(1025, 2), (1025, 3), (2049, 1)}
    assert all((g, s) in SHAPES for s in SIZES for g in (1, 3, 67)) and len(SHAPES) == 7 * 3 + 3
    rows = sum(g * s * (12 if g <= 3 else 3) for g, s in SHAPES)
    assert rows == 328 * 4 * 12 + (328 * 67 + 2050 + 3075 + 2049) * 3 == 103194


def test_blocks_of_several_waves_change_base(eng):
    """Blocks grow past 64 lanes only when 64-lane blocks cannot hold the rows in one pass over the chip: from 16 385 rows on 256 CUs in the
    default mode, from 65 537 in constant-time mode (four 256-lane blocks per CU).  These are the smallest shapes with 130 bases beyond that;
    their blocks are two waves wide and most of them change base inside their item range (tests/test_commit_oracle.py), so a wave may still
    read the comb that another is about to replace: what the barrier in front of the staging is for."""
    c = main_set(eng)
    groups, size = WIDE[eng.ct_select]
    check(dev_call(eng, c["k_words"][:groups * size], groups, size, 1), expected(eng, groups, size)[0])


# ---- 2. parity with the ladder route over the tiled bases, and with the fixture ------------------------------------------------------------
@pytest.mark.parametrize("groups,size", [(3, 65), (67, 3)])
def test_bytes_equal_msm_over_the_tiled_bases(eng, groups, size):
    c = main_set(eng)
    k = c["k_words"][:groups * size]
    tiled = np.tile(c["B"][:size], (groups, 1))
    want = eng.msm(k, tiled, size)
    want_enc, st = eng.msm_bytes(k, oc.encode(tiled), size)
    assert not st.any()
    check(want, expected(eng, groups, size)[0])
    for route in ROUTES:
        assert eng.commit(k, size, route).tobytes() == want.tobytes()
        assert eng.commit_bytes(k, size, route).tobytes() == want_enc.tobytes()


def test_fixture_made_with_the_reference(eng):
    raw = load_golden("commit.json", raw=True)
    num = lambda P: tuple(tuple(int(x, 16) for x in coord) for coord in P)
    use_set(eng, "fixture", codec.pack_points([num(B) for B in raw["bases"]], 2))
    assert eng.commit_bases_count == 5
    for case in raw["cases"]:
        size = case["group_size"]
        k = codec.pack_scalars([int(x, 16) for g in case["groups"] for x in g["k"]])
        want = codec.pack_points([num(g["affine"]) for g in case["groups"]], 2)
        want_enc = np.array([list(bytes.fromhex(g["enc"])) for g in case["groups"]], dtype=np.uint8)
        for route in ROUTES:
            check(eng.commit(k, size, route), want)
            check(dev_call(eng, k, len(want), size, route, encoded=True), want_enc)
    assert np.array_equal(want[0], NEUTRAL_AFFINE) and np.array_equal(want_enc[0], NEUTRAL_ENC)     # the last case commits to the neutral


# ---- 3. neutral results ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_neutral_results(eng, route):
    c = main_set(eng)
    for groups, size in ((1, 1), (3, 2), (2, 65)):                                           # all scalars zero
        zeros = np.zeros((groups * size, 4), dtype=np.uint64)
        check(eng.commit(zeros, size, route), np.tile(NEUTRAL_AFFINE, (groups, 1)))
        check(dev_call(eng, zeros, groups, size, route, encoded=True), np.tile(NEUTRAL_ENC, (groups, 1)))
    for size in (2, 5, 66):                                                                   # sum k t = 0 (mod N), beside an ordinary group
        ks = c["k"][100:100 + size - 1]
        ks = ks + [ref.closing_scalar(ks, c["t"])] + c["k"][:size]
        assert sum(k * t for k, t in zip(ks[:size], c["t"])) % o.N == 0
        want, want_enc = multiples_of_g(c, [0, sum(k * t for k, t in zip(ks[size:], c["t"]))])
        assert np.array_equal(want[0], NEUTRAL_AFFINE) and np.array_equal(want_enc[0], NEUTRAL_ENC) and not np.array_equal(want[1], NEUTRAL_AFFINE)
        check(eng.commit(codec.pack_scalars(ks), size, route), want)
        check(eng.commit_bytes(codec.pack_scalars(ks), size, route), want_enc)


def test_a_base_twice_and_a_base_with_its_negative(eng):
    """The set (B, B, -B): equal scalars on the first two add a point to itself, equal scalars on B and -B give the neutral -- both through
    the complete addition of the fold."""
    c = pool(eng)
    B = codec.unpack_points(c["B"][:1])[0]
    minus = (tuple((P127 - v) % P127 for v in B[0]), B[1])
    assert o.PointOnCurve(minus) and ref.multiple_of_g(o.N - c["t"][0]) == minus
    ts = [c["t"][0], c["t"][0], o.N - c["t"][0]]
    try:
        use_set(eng, "twice", codec.pack_points([B, B, minus], 2))
        k = c["k"][40]
        groups = [[k, k, 0], [k, 0, k], [0, k, k], [k, k, 2 * k % o.N], [k, k, k]]
        want, want_enc = multiples_of_g(c, [sum(x * t for x, t in zip(g, ts)) for g in groups])
        assert [bool(np.array_equal(w, NEUTRAL_AFFINE)) for w in want] == [False, True, True, True, False]
        flat = codec.pack_scalars([x for g in groups for x in g])
        for route in ROUTES:
            check(eng.commit(flat, 3, route), want)
            check(dev_call(eng, flat, len(groups), 3, route, encoded=True), want_enc)
        check(eng.commit(codec.pack_scalars([k, k]), 2), multiples_of_g(c, [2 * k * ts[0]])[0])
    finally:
        main_set(eng)


# ---- 4. the set ------------------------------------------------------------------------------------------------------------------------------
def test_set_handling(eng):
    c = main_set(eng)
    import torch
    eng.comb_stage(eng.comb_table(G1_WORDS))
    kd = to_dev(c["k_words"][:70])

    def staged_comb():
        """[k]G through comb_mul_dev with comb_host=None: the comb staged by comb_stage"""
        out = torch.zeros((70, 8), dtype=torch.int64, device=kd.device)
        st = torch.full((70,), 0xA5, dtype=torch.uint8, device=kd.device)
        eng.comb_mul_dev(kd, None, out, st, 70)
        eng.sync()
        return out.cpu().numpy().view(np.uint64), st.cpu().numpy()
    before, st = staged_comb()
    k = c["k_words"][:6]
    first = eng.commit(k, 3)
    check(first, expected(eng, 2, 3)[0])                                                     # a shorter vector uses the first bases
    use_set(eng, "reversed", c["B"][::-1][:7])                                                # another set: no stale array
    assert eng.commit_bases_count == 7
    t_rev = c["t"][::-1][:7]
    want = multiples_of_g(c, [sum(c["k"][g * 3 + j] * t_rev[j] for j in range(3)) for g in range(2)])[0]
    second = eng.commit(k, 3)
    check(second, want)
    assert mismatches(first, second).size == 2
    with pytest.raises(_lib.FourQError):                                                      # above the new set's size
        eng.commit(c["k_words"][:8], 8)
    after, st2 = staged_comb()                                                                # the staged generator comb still answers as before
    assert np.array_equal(before, after) and np.array_equal(st, st2)
    ok = st == 0                                                                              # the comb call reports the neutral in its status
    assert [i for i in range(70) if not ok[i]] == [i for i in range(70) if c["k"][i] % o.N == 0] and ok.sum() >= 60
    assert np.array_equal(before[ok], oc.r1_to_affine(oc.mul(oc.ENDO, c["k_words"][:70], None, c["table"]))[ok])
    for bad in (np.zeros((0, 8), dtype=np.uint64), np.zeros((4097, 8), dtype=np.uint64)):    # a failed call keeps the old set
        with pytest.raises(_lib.FourQError):
            eng.commit_bases(bad)
        assert eng.commit_bases_count == 7
        check(eng.commit(k, 3), want)
    main_set(eng)
    check(eng.commit(k, 3), first)


def test_generators_from_hash_to_curve(eng):
    """commit_generators: hash_to_curve(I2OSP(j, 4), dst) -- order N by construction; the commitment equals the ladder route's over them."""
    c = pool(eng)
    dst = b"fourq_amd commitment generators, test"
    gens = eng.commit_generators(4, dst)
    msgs = np.array([[0, 0, 0, j] for j in range(4)], dtype=np.uint8)
    assert np.array_equal(gens, eng.hash_to_curve(msgs, dst=dst, affine=True)) and len({g.tobytes() for g in gens}) == 4
    lifted = np.concatenate([gens, np.tile(codec.pack_fp2s([(1, 0)]), (4, 1)), gens], axis=1)
    n_times = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars([o.N] * 4), lifted))
    check(n_times, np.tile(NEUTRAL_AFFINE, (4, 1)))                                           # [N]B = O, by the C oracle
    try:
        use_set(eng, "hashed", gens)
        k = c["k_words"][:12]
        want = oc.r1_to_affine(oc.mul(oc.ENDO, k, np.tile(lifted, (3, 1))))
        acc = [None] * 3
        pts = codec.unpack_points(want)
        for i, P in enumerate(pts):
            T = o.AffineToR1(*P)
            acc[i // 4] = T if acc[i // 4] is None else o.ADD(acc[i // 4], o.R1toR2(T))
        want = codec.pack_points([o.R1toAffine(a) for a in acc], 2)
        for route in ROUTES:
            check(eng.commit(k, 4, route), want)
        assert eng.commit(k, 4).tobytes() == eng.msm(k, np.tile(gens, (3, 1)), 4).tobytes()
    finally:
        main_set(eng)


# ---- 5. sequences -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [False, True], ids=["unreserved", "reserved"])
def test_two_unsynchronised_dev_calls(eng, reserve):
    c = main_set(eng)
    if reserve:
        eng.commit_reserve(67, 65)
    shapes = [(67, 65, 1, False), (3, 130, 2, True)] if reserve else [(3, 64, 2, True), (67, 3, 1, False)]
    pending = [dev_call(eng, c["k_words"][:g * s], g, s, route, encoded=enc, sync=False) + (g, s, enc) for g, s, route, enc in shapes]
    eng.sync()
    for read, _, g, s, enc in pending:
        check(read(), expected(eng, g, s)[1 if enc else 0])


# ---- 6. the argument contract -------------------------------------------------------------------------------------------------------------------
def test_argument_contract(eng):
    import torch
    c = main_set(eng)
    lib, ctx, INVALID = eng._lib, eng._ctx, _lib.ERR_INVALID
    dev = torch.device("cuda", 0)
    k = to_dev(c["k_words"][:8])
    out = torch.full((6, 64), 0xA5, dtype=torch.uint8, device=dev)
    hk, hout = c["k_words"][:8].copy(), np.full((4, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    p = lambda x: ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    calls = [(lib.fourq_commit_affine_dev, p(k), p(out)), (lib.fourq_commit_bytes_dev, p(k), p(out)),
             (lib.fourq_commit_affine, p(hk), p(hout)), (lib.fourq_commit_bytes, p(hk), p(hout))]
    for fn, pk, po in calls:
        assert fn(None, pk, po, 4, 2, 0) == INVALID                                          # a NULL context, everything else valid
        assert fn(ctx, pk, po, 4, 0, 0) == INVALID                                           # group_size == 0
        assert fn(ctx, pk, po, 1, BASES + 1, 0) == INVALID                                   # above the set's size
        assert fn(ctx, pk, po, _lib.MAX_BATCH // 2 + 1, 2, 0) == INVALID                     # groups x group_size above FOURQ_MAX_BATCH
        assert fn(ctx, pk, po, 1 << 63, 2, 0) == INVALID                                     # ... also where the product wraps to 0
        assert fn(ctx, pk, po, ((1 << 64) - 1) // 3 + 1, 3, 0) == INVALID                    # ... or to a small number
        for route in (-1, 3, 1 << 20):
            assert fn(ctx, pk, po, 4, 2, route) == INVALID
        assert fn(ctx, None, po, 4, 2, 0) == INVALID and fn(ctx, pk, None, 4, 2, 0) == INVALID
        assert fn(ctx, pk, po, 0, 2, 0) == _lib.OK and fn(ctx, pk, po, 0, 0, 1) == _lib.OK   # groups == 0: nothing touched
    for fn in (lib.fourq_commit_affine_dev, lib.fourq_commit_bytes_dev):                     # a misaligned _dev pointer, either one
        assert fn(ctx, ctypes.c_void_p(k.data_ptr() + 8), p(out), 3, 2, 0) == INVALID
        assert fn(ctx, p(k), ctypes.c_void_p(out.data_ptr() + 8), 3, 2, 0) == INVALID
    eng.sync()
    assert (out.cpu().numpy() == 0xA5).all() and (hout == 0xA5A5A5A5A5A5A5A5).all()
    assert lib.fourq_commit_reserve(ctx, 0, 0) == _lib.OK
    assert lib.fourq_commit_reserve(ctx, 1, 0) == INVALID and lib.fourq_commit_reserve(ctx, 1 << 63, 2) == INVALID
    assert lib.fourq_commit_bases_set(ctx, None, 1) == INVALID and lib.fourq_commit_bases_count(ctx, None) == INVALID
    assert eng.commit_bases_count == BASES
    check(dev_call(eng, c["k_words"][:8], 4, 2, 0), expected(eng, 4, 2)[0])                  # ... and the context still works
    fresh = Engine(0)                                                                         # no set present
    try:
        fresh.ct_select = eng.ct_select
        assert fresh.commit_bases_count == 0
        for fn, pk, po in calls:
            assert fn(fresh._ctx, pk, po, 1, 1, 0) == INVALID and fn(fresh._ctx, pk, po, 0, 1, 0) == _lib.OK
    finally:
        fresh.close()


# ---- 7. all devices behind one call ----------------------------------------------------------------------------------------------------------
def test_multi_engine_with_one_device_equals_engine(eng):
    c = main_set(eng)
    k = c["k_words"][:67 * 3]
    with MultiEngine([0]) as multi:
        multi.ct_select = eng.ct_select
        multi.commit_bases(c["B"][:5])
        assert multi.commit_bases_count == 5
        for route in ROUTES:
            assert multi.commit(k, 3, route).tobytes() == eng.commit(k, 3, route).tobytes()
            assert multi.commit_bytes(k, 3, route).tobytes() == eng.commit_bytes(k, 3, route).tobytes()
    with MultiEngine([0, 0]) as multi:                                                       # two contexts: whole groups are sharded
        multi.ct_select = eng.ct_select
        multi.commit_bases(c["B"][:5])
        check(multi.commit(k, 3), expected(eng, 67, 3)[0])
        check(multi.commit_bytes(k, 3), expected(eng, 67, 3)[1])
