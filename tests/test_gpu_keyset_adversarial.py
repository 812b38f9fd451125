"""The key set (fourq_keyset_*, fourq_amd/csrc/keyset.hip.h) under keys its caller does not choose: tests/keyset_adversarial.py's families
registered as keys, the structured keys whose rows steer the two-combs-in-one-accumulator walk into every special case of the complete
addition, the set at its documented size and its replacement across the block edge of the one-lane-per-key kernels, and -- through the same
build_combs -- commitment bases with a half of x that is 0.

Expected values never come from the code under test.  Key statuses: keyset_ref.key_status (pinned to the real reference by
tests/golden/keyset_adversarial.json on the CPU).  Rows under keys [t]G with known t: the group law, out = [(k + l t) mod N]G with the sum in
Python integers and the point from the C oracle.  Rows under the six accepted strings without a known logarithm: keyset_ref's restatement
on the Python oracle.  Every test takes `eng`: selection by address (keyset_comb_kernel) and constant-time selection (the unkeyed routes on
the gathered key bytes plus keyset_fix_kernel) must give the same bytes.  _dev outputs go into 0xA5-filled tensors two rows longer than
needed, and the tail is checked."""
import random

import numpy as np
import pytest

import adversarial_points as adv
import bucket_ref
import curve4q_oracle as o
import keyset_adversarial as ka
import keyset_ref as kref
import oracle_c as oc
import sig_ref as ref
from fourq_amd import _lib, codec
from test_gpu_sig import bad_rows, byte_rows, g_comb

pytestmark = pytest.mark.gpu

N = o.N
REFUSED = kref.KEYSET_NOT_ORDER_N
POOL = 4096
LENGTHS = [0, 1, 15, 16, 17, 47, 48, 79, 80, 111, 112, 127, 128, 129, 200]
_cache = {}


def pool():
    """POOL honest keys: (sks, ts, pks) with pks[j] = encode([ts[j]]G) from the C oracle; per session"""
    if "pool" not in _cache:
        raw = np.random.default_rng(7810).integers(0, 256, size=(POOL, 32), dtype=np.uint8)
        sks = [r.tobytes() for r in raw]
        ts = [ref.LE(ref.H(sk)[:32]) % N for sk in sks]
        pks = ref.batch_keygen(sks)
        assert len({p.tobytes() for p in pks}) == POOL
        _cache["pool"] = (sks, ts, pks)
    return _cache["pool"]


def seeded_scalars(n, seed):
    """two lists of n seeded 256-bit scalars with the six edge values planted in each, at different rows"""
    rng = random.Random(seed)
    k = bucket_ref.plant_edges([rng.getrandbits(256) for _ in range(n)])
    l = [rng.getrandbits(256) for _ in range(n)]
    for i, e in enumerate(bucket_ref.EDGE_SCALARS):
        l[(3 + 11 * i) % n] = e
        l[(n - 2 - 13 * i) % n] = e
    return k, l


def messages(n, seed):
    rng = random.Random(seed)
    blob = np.random.default_rng(seed).integers(0, 256, size=1 << 12, dtype=np.uint8).tobytes()
    out = []
    for i in range(n):
        at = rng.randrange(len(blob) - 256)
        out.append(blob[at:at + LENGTHS[i % len(LENGTHS)]])
    return out


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


def guarded(n, width=None):
    import torch
    return torch.full((n + 2,) if width is None else (n + 2, width), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))


def unguard(t, n):
    got = t.cpu().numpy()
    assert (got[n:] == 0xA5).all()
    return got[:n]


def dev_double_mul(e, k, l, ids):
    n = len(ids)
    out, st = guarded(n, 32), guarded(n)
    e.keyset_double_mul_bytes_dev(to_dev(k), to_dev(l), to_dev(np.asarray(ids, dtype=np.uint32)), out, st, n)
    e.sync()
    return unguard(out, n), unguard(st, n)


def dev_verify(e, ids, matrix, lens, sigs):
    n = len(ids)
    ok, st = guarded(n), guarded(n)
    e.sig_verify_keyed_dev(to_dev(np.asarray(ids, dtype=np.uint32)), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, to_dev(sigs), ok, st, n)
    e.sync()
    return unguard(ok, n), unguard(st, n)


def expected_rows(ids, ks, ls, slot_t, slot_st, count, special=None):
    """(out, status) of the keyed double multiplication: a zero row and the status for an index outside the set or a refused slot, the
    group law for a slot with a known logarithm, special[row] = (bytes, status) for the others"""
    n = len(ids)
    st = np.array([kref.KEYSET_ID_RANGE if i >= count else slot_st[i] for i in ids], dtype=np.uint8)
    known = [r for r in range(n) if not st[r] and slot_t[ids[r]] is not None]
    out = np.zeros((n, 32), dtype=np.uint8)
    out[known] = ka.group_law_bytes([ks[r] for r in known], [ls[r] for r in known], [slot_t[ids[r]] for r in known])
    for r in range(n):
        if not st[r] and slot_t[ids[r]] is None:
            b, s = special[r]
            assert s == 0
            out[r] = np.frombuffer(b, dtype=np.uint8)
    return out, st


def check_double_mul(e, ids, ks, ls, want_out, want_st, host=True, what=""):
    k, l = codec.pack_scalars(ks), codec.pack_scalars(ls)
    calls = [("_dev", lambda: dev_double_mul(e, k, l, ids))]
    if host:
        calls.insert(0, ("host", lambda: e.keyset_double_mul_bytes(k, l, np.asarray(ids, dtype=np.uint32))))
    for form, call in calls:
        out, st = call()
        bad = bad_rows(out, want_out)
        assert bad.size == 0, (what, form, [(int(r), int(ids[r]), hex(ks[r]), hex(ls[r])) for r in bad[:6]])
        assert np.array_equal(st, want_st), (what, form, [(int(r), int(ids[r]), int(st[r]), int(want_st[r])) for r in np.flatnonzero(st != want_st)[:6]])
    return k, l


def check_verify(e, ids, msgs, sigs, want_ok, want_st, what=""):
    matrix, lens = codec.pack_messages(msgs)
    for form, call in (("host", lambda: e.sig_verify_keyed(np.asarray(ids, dtype=np.uint32), matrix, sigs, lens)), ("_dev", lambda: dev_verify(e, ids, matrix, lens, sigs))):
        ok, st = call()
        assert np.array_equal(st, want_st), (what, form, [(int(r), int(ids[r]), int(st[r]), int(want_st[r])) for r in np.flatnonzero(st != want_st)[:6]])
        assert np.array_equal(ok, want_ok), (what, form, [(int(r), int(ids[r])) for r in np.flatnonzero(ok != want_ok)[:6]])


def sign_rows(cs, pks, msgs, seed):
    """(n, 64) signatures under the keys [c_i]G from their logarithms: R = [r]G from the C oracle, s = r - c h mod N"""
    rng = random.Random(seed)
    rs = [rng.randrange(1, N) for _ in cs]
    R = ka.multiples_of_g(rs)
    out = np.empty((len(cs), 64), dtype=np.uint8)
    out[:, :32] = R
    for i, (c, pk, msg) in enumerate(zip(cs, pks, msgs)):
        s = (rs[i] - c * ref.challenge(R[i].tobytes(), bytes(pk), msg)) % N
        out[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint8)
    return out


# ---- D1. every adversarial string in a slot of its own, an honest key beside each ------------------------------------------------------------
def test_every_string_as_a_registered_key(eng):
    fam = ka.strings()
    sks, ts, pks = pool()
    f = len(fam)
    m = 2 * f
    assert m == 2244
    keys = np.empty((m, 32), dtype=np.uint8)
    keys[0::2] = byte_rows([b for _, b in fam], 32)
    keys[1::2] = pks[:f]
    key_list = [r.tobytes() for r in keys]
    slot_st = np.zeros(m, dtype=np.uint8)
    slot_st[0::2] = ka.key_statuses([b for _, b in fam])
    slot_t = [None if j % 2 == 0 else ts[j // 2] for j in range(m)]
    accepted = [j for j in range(0, m, 2) if slot_st[j] == 0]
    assert len(accepted) == 6
    g_comb(eng)
    got = eng.keyset_set(keys)
    wrong = np.flatnonzero(got != slot_st)
    assert wrong.size == 0, [(fam[j // 2][0] if j % 2 == 0 else "honest %d" % (j // 2), int(got[j]), int(slot_st[j])) for j in wrong[:8]]
    assert eng.keyset_count() == m

    # scalar rows: every slot named twice
    perm = np.random.default_rng(7820).permutation(m).astype(np.uint32)
    ids = np.concatenate([perm, perm])
    n = len(ids)
    ks, ls = seeded_scalars(n, 7821)
    special = {r: kref.double_mul_keyed(key_list, int(ids[r]), ks[r], ls[r]) for r in range(n) if ids[r] in accepted}
    assert len(special) == 12
    want_out, want_st = expected_rows(ids, ks, ls, slot_t, slot_st, m, special)
    refused = want_st != 0
    assert not want_out[refused].any() and want_out[~refused].any(axis=1).all() and refused.sum() == 2 * (f - 6)
    k, l = check_double_mul(eng, ids, ks, ls, want_out, want_st, what="strings")
    # the header's contract, a cross-check between two device routes: for an accepted key, the unkeyed call on keys[ids]
    live = np.flatnonzero(~refused)
    out, st = eng.double_mul_bytes(k[live], l[live], keys[ids[live]])
    assert bad_rows(out, want_out[live]).size == 0 and not st.any()

    # verify rows: one honest signature per honest slot; a third of them, and one more per accepted string, named to the string slot beside
    order = np.random.default_rng(7822).permutation(f)
    signer = list(order) + [j // 2 for j in accepted]
    v = len(signer)
    msgs = messages(v, 7823)
    sigs = ref.batch_sign([sks[i] for i in signer], [pks[i] for i in signer], msgs)
    vids = np.array([2 * i + 1 for i in signer], dtype=np.uint32)
    vids[0:f:3] -= 1
    vids[f:] -= 1
    assert set(accepted) <= set(vids[f:])
    want_ok, want_vst = np.ones(v, dtype=np.uint8), np.zeros(v, dtype=np.uint8)
    for r in np.flatnonzero(vids % 2 == 0):
        j = int(vids[r])
        want_ok[r], want_vst[r] = (0, slot_st[j]) if slot_st[j] else kref.verify_keyed(key_list, j, msgs[r], sigs[r].tobytes())
    assert want_ok.sum() == f - len(range(0, f, 3))                                          # every undisturbed row, and no other
    check_verify(eng, vids, msgs, sigs, want_ok, want_vst, what="strings")


# ---- D2. keys of order 4N, 7N, ... 56N, and 2N --------------------------------------------------------------------------------------------
def test_keys_of_order_a_multiple_of_n_are_refused(eng):
    fam = ka.shifted()
    honest = ka.honest_shift_strings()
    hts = [t for t, _ in ka.shift_keys()]
    f = len(fam)
    m = 2 * f
    assert m < 256
    keys = np.empty((m, 32), dtype=np.uint8)
    keys[0::2] = byte_rows([b for _, b in fam], 32)
    keys[1::2] = byte_rows([honest[i % 3] for i in range(f)], 32)
    slot_st = np.tile(np.array([REFUSED, 0], dtype=np.uint8), f)
    slot_t = [None if j % 2 == 0 else hts[(j // 2) % 3] for j in range(m)]
    g_comb(eng)
    got = eng.keyset_set(keys)
    wrong = np.flatnonzero(got != slot_st)
    assert wrong.size == 0, [(fam[j // 2][0] if j % 2 == 0 else "honest", int(got[j])) for j in wrong[:8]]
    assert eng.keyset_count() == m
    n = 500
    rng = np.random.default_rng(7830)
    ids = np.concatenate([rng.permutation(m), rng.integers(0, m, size=n - m)]).astype(np.uint32)
    ks, ls = seeded_scalars(n, 7831)
    want_out, want_st = expected_rows(ids, ks, ls, slot_t, slot_st, m)
    assert set(want_st) == {0, REFUSED} and not want_out[want_st != 0].any()
    check_double_mul(eng, ids, ks, ls, want_out, want_st, what="shifted")
    # signatures of the honest key beside (or in) the slot: accepted under the honest slot, ok = 0 and status 96 under the shifted one
    msgs = messages(n, 7832)
    who = [(int(j) // 2) % 3 for j in ids]
    sigs = sign_rows([hts[w] for w in who], [honest[w] for w in who], msgs, 7833)
    check_verify(eng, ids, msgs, sigs, (want_st == 0).astype(np.uint8), want_st, what="shifted")


# ---- D3. keys that are known multiples of G: the special cases of the complete addition inside the walk -----------------------------------
def test_structured_keys_reach_every_state_of_the_walk(eng):
    fam = ka.structured()
    rows = ka.structured_rows()
    m = len(fam)
    assert m == 8
    keys = byte_rows([b for _, b in fam], 32)
    g_comb(eng)
    assert not eng.keyset_set(keys).any() and eng.keyset_count() == m
    slot_t, slot_st = list(ka.STRUCTURED_C), np.zeros(m, dtype=np.uint8)
    base_out, _ = expected_rows([j for j, _, _, _ in rows], [k for _, k, _, _ in rows], [l for _, _, l, _ in rows], slot_t, slot_st, m)
    neutral = [r for r, (j, k, l, _) in enumerate(rows) if (k + l * slot_t[j]) % N == 0]
    assert len(neutral) >= m and all(base_out[r].tobytes() == kref.NEUTRAL_BYTES for r in neutral)
    for n in (len(rows), 257, 1025):                                                         # all rows; a tail lane; several blocks
        pick = [r % len(rows) for r in range(n)]
        ids = np.array([rows[r][0] for r in pick], dtype=np.uint32)
        ks, ls = [rows[r][1] for r in pick], [rows[r][2] for r in pick]
        k, l = codec.pack_scalars(ks), codec.pack_scalars(ls)
        for form, (out, st) in (("host", eng.keyset_double_mul_bytes(k, l, ids)), ("_dev", dev_double_mul(eng, k, l, ids))):
            bad = bad_rows(out, base_out[pick])
            assert bad.size == 0, (form, n, [(fam[rows[pick[r]][0]][0], rows[pick[r]][3], hex(ks[r]), hex(ls[r]), ka.parities(ks[r], ls[r])) for r in bad[:8]])
            assert not st.any(), (form, n)
    # one valid signature per key from its logarithm; one flipped bit of s
    msgs = messages(m, 7840)
    sigs = sign_rows(slot_t, [b for _, b in fam], msgs, 7841)
    ids = np.arange(m, dtype=np.uint32)
    for pk, msg, sig in zip(keys, msgs, sigs):
        assert ref.verify(pk.tobytes(), msg, sig.tobytes()) == (1, 0)                        # the restatement accepts them
    check_verify(eng, ids, msgs, sigs, np.ones(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8), what="structured, valid")
    flipped = sigs.copy()
    flipped[:, 32 + 9] ^= 0x10
    want_st = np.array([ref.SIG_S_RANGE if ref.LE(s[32:].tobytes()) >= N else 0 for s in flipped], dtype=np.uint8)
    check_verify(eng, ids, msgs, flipped, np.zeros(m, dtype=np.uint8), want_st, what="structured, one bit of s flipped")


# ---- D4. the set at its documented size, and smaller sets after it ------------------------------------------------------------------------
def test_the_largest_set_and_its_replacement(eng):
    from fourq_amd import Engine, FourQError
    sks, ts, pks = pool()
    fam = ka.strings()
    undecodable = next(b for (_, b), s in zip(fam, ka.key_statuses([b for _, b in fam])) if s == ref.BYTES_DECODE_BASE + ref.DECODE_NOT_ON_CURVE)
    shifted = [b for _, b in ka.shifted()]
    NOT_ON_CURVE = ref.BYTES_DECODE_BASE + ref.DECODE_NOT_ON_CURVE

    def build(first, m, planted):
        """pool keys first .. first + m - 1 with planted = {slot: (bytes, status)}: (keys, slot_t, slot_st)"""
        keys = pks[first:first + m].copy()
        slot_t, slot_st = list(ts[first:first + m]), np.zeros(m, dtype=np.uint8)
        for j, (b, s) in planted.items():
            keys[j], slot_t[j], slot_st[j] = np.frombuffer(b, dtype=np.uint8), None, s
        return keys, slot_t, slot_st

    with Engine(0) as e:
        e.ct_select = eng.ct_select
        e.comb_stage(e.comb_table(codec.pack_point(ref.G1)))
        m = _lib.KEYSET_MAX_KEYS
        assert m == POOL == 4096
        keys, slot_t, slot_st = build(0, m, {256: (undecodable, NOT_ON_CURVE), 4094: (shifted[5], REFUSED)})
        got = e.keyset_set(keys)
        assert np.array_equal(got, slot_st), np.flatnonzero(got != slot_st)[:8]
        assert e.keyset_count() == m and slot_st[4095] == 0
        ids = np.concatenate([np.random.default_rng(7850).permutation(m), np.resize([4095, 4094, 0, 2048], 77)]).astype(np.uint32)
        n = len(ids)
        ks, ls = seeded_scalars(n, 7851)
        want_out, want_st = expected_rows(ids, ks, ls, slot_t, slot_st, m)
        assert (want_st != 0).sum() == 1 + 1 + 19 and want_out[want_st == 0].any(axis=1).all()
        check_double_mul(e, ids, ks, ls, want_out, want_st, what="4096 keys")

        # a smaller set, one key past a block of the one-lane-per-key kernels; the old indices name the new keys or nothing
        keys, slot_t, slot_st = build(1000, 257, {256: (shifted[40], REFUSED)})
        got = e.keyset_set(keys)
        assert np.array_equal(got, slot_st) and e.keyset_count() == 257
        ids = np.concatenate([np.random.default_rng(7852).permutation(257), [256, 0, 255]]).astype(np.uint32)
        ks, ls = seeded_scalars(len(ids), 7853)
        want_out, want_st = expected_rows(ids, ks, ls, slot_t, slot_st, 257)
        assert list(want_st[ids == 256]) == [REFUSED, REFUSED]
        check_double_mul(e, ids, ks, ls, want_out, want_st, what="257 keys")
        far = ids.copy()
        far[3::50] = 257
        far[4::50] = 4095
        want_out, want_st = expected_rows(far, ks, ls, slot_t, slot_st, 257)
        assert (want_st == kref.KEYSET_ID_RANGE).sum() == 12 and not want_out[want_st != 0].any()
        k, l = check_double_mul(e, far, ks, ls, want_out, want_st, host=False, what="257 keys, indices outside")
        with pytest.raises(FourQError):
            e.keyset_double_mul_bytes(k, l, far)

        # ... and exactly one block
        keys, slot_t, slot_st = build(2000, 256, {255: (undecodable, NOT_ON_CURVE)})
        got = e.keyset_set(keys)
        assert np.array_equal(got, slot_st) and e.keyset_count() == 256
        ids = np.concatenate([np.random.default_rng(7854).permutation(256), [255, 254, 0]]).astype(np.uint32)
        ks, ls = seeded_scalars(len(ids), 7855)
        want_out, want_st = expected_rows(ids, ks, ls, slot_t, slot_st, 256)
        check_double_mul(e, ids, ks, ls, want_out, want_st, what="256 keys")
        far = ids.copy()
        far[7] = 256
        want_out, want_st = expected_rows(far, ks, ls, slot_t, slot_st, 256)
        check_double_mul(e, far, ks, ls, want_out, want_st, host=False, what="256 keys, index 256")


# ---- D5. the same build_combs from unchecked affine words: bases with a half of x that is 0 ---------------------------------------------------
def test_commit_bases_with_a_zero_half(eng):
    """commit_bases takes affine words as they are, so it can be given what no string delivers: all eight subgroup points with x0 = 0 or
    x1 = 0 (the encodings of the four with x0 = 0 do not decode), and G and -G.  Expected: the C oracle's MUL_endo row per element, chained
    with the Python oracle's complete ADD."""
    import torch
    half = adv.subgroup_zero_half()
    assert len(half) == 8 and sum(1 for _, (x, _) in half if x[0] == 0) == 4 and sum(1 for _, (x, _) in half if x[1] == 0) == 4
    bases = [pt for _, pt in half] + [ka.G, (o.f2_neg(o.Gx), o.Gy)]
    assert all(o.PointOnCurve(pt) for pt in bases)
    size, most = len(bases), 67
    P = codec.pack_points(bases, 2)
    rng = random.Random(7860)
    scalars = bucket_ref.plant_edges([rng.getrandbits(256) for _ in range(most * size)])
    same = rng.getrandbits(256)
    scalars[size:2 * size] = [0] * 8 + [same, same]                                          # group 1: [same]G + [same](-G)
    k = codec.pack_scalars(scalars)
    lifted = np.zeros((most * size, 20), dtype=np.uint64)
    lifted[:, 0:8], lifted[:, 8], lifted[:, 12:20] = np.tile(P, (most, 1)), 1, np.tile(P, (most, 1))
    products = codec.unpack_points(oc.mul(oc.ENDO, k, lifted))
    sums = []
    for g in range(most):
        acc = products[g * size]
        for B in products[g * size + 1:(g + 1) * size]:
            acc = o.ADD(acc, o.R1toR2(B))
        sums.append(o.R1toAffine(acc))
    want = codec.pack_points(sums, 2)
    want_enc = byte_rows([bytes(o.encode(*s)) for s in sums], 32)
    assert sums[1] == adv.NEUTRAL and want_enc[1].tobytes() == kref.NEUTRAL_BYTES and sums[0] != adv.NEUTRAL
    eng.commit_bases(P)
    assert eng.commit_bases_count == size
    for route in (1, 2, 0):
        for groups in (1, 3, most):
            rows = k[:groups * size]
            got = eng.commit(rows, size, route)
            assert bad_rows(got, want[:groups]).size == 0, (route, groups, bad_rows(got, want[:groups])[:8])
            got = eng.commit_bytes(rows, size, route)
            assert bad_rows(got, want_enc[:groups]).size == 0, (route, groups, bad_rows(got, want_enc[:groups])[:8])
            out = torch.full((groups + 2, 32), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
            eng.commit_bytes_dev(to_dev(rows), out, groups, size, route)
            eng.sync()
            assert bad_rows(unguard(out, groups), want_enc[:groups]).size == 0, (route, groups, "_dev")
