"""The calls that are built from other calls, while the context's buffers grow under them (fourq_amd.hip, WorkScope; work_layout.h, the rule).
A composite call keeps values in the work buffer across the calls it makes -- three deep in keyed VRF verify and, with constant-time
selection, in keyed signature verify -- so an inner call that moved the buffer would lose them and still return FOURQ_OK.

Every test here runs its calls on a fresh context with nothing reserved, at 1, then 33, then 300 rows, enqueued without a synchronisation in
between into separate pre-filled outputs: each step outgrows the quarter of headroom the step before left, so the OUTERMOST call of each step
reallocates while its predecessors are in flight, and no inner call may.  One synchronisation at the end.  Every output must be byte-equal to
the same calls on a second context that was reserved first and synchronised after every call, and say what the feature tests expect: ok = 1
on every row but the one whose signature or proof was corrupted in one byte, with status 0 there (the proof does not hold; nothing fails to
decode).  The signatures and proofs are honest ones made on the device, by the reserved context.  Both selection modes."""
import numpy as np
import pytest

from test_gpu_dleq import G1_WORDS

pytestmark = pytest.mark.gpu

STEPS = (1, 33, 300)
DLEQ_SHAPES = ((1, 1), (3, 11), (5, 60))        # (groups, group_size): 1, 33 and 300 rows
TOP = STEPS[-1]
STRIDE = 75                                     # no multiple of 8: rows are read by bytes
DST = b"FourQ-work-hold-tests"
KEYS = 3
_comb = []


def filled(*shape):
    import torch
    return torch.full(shape, 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))


def host(t):
    return t.cpu().numpy()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


@pytest.fixture()
def pair(eng):
    """(fresh, reserved): two new contexts in `eng`'s selection mode with the generator's comb staged; the second one reserved at the top size"""
    import torch
    from fourq_amd import Engine
    if not _comb:
        _comb.append(eng.comb_table(G1_WORDS))
    with Engine(0) as fresh, Engine(0) as reserved:
        for e in (fresh, reserved):
            e.ct_select = eng.ct_select
            e.comb_stage(_comb[0])
        reserved.reserve(TOP)
        reserved.keyset_reserve(TOP)
        reserved.dleq_reserve(*DLEQ_SHAPES[-1])
        reserved.vrf_reserve(TOP)
        yield fresh, reserved
        torch.cuda.synchronize()


def rows(seed):
    """secret keys of KEYS signers spread over TOP rows by index, ragged messages, and two scalars per row"""
    rng = np.random.default_rng(seed)
    ids = (np.arange(TOP) % KEYS).astype(np.uint32)
    sk3 = rng.integers(0, 256, size=(KEYS, 32), dtype=np.uint8)
    matrix = rng.integers(0, 256, size=(TOP, STRIDE), dtype=np.uint8)
    lens = rng.integers(0, STRIDE + 1, size=TOP).astype(np.uint32)
    scalars = rng.integers(0, 1 << 63, size=(2, TOP, 4), dtype=np.uint64)
    return ids, sk3, matrix, lens, scalars


def registered(fresh, reserved, sk3):
    """the signers' public keys, made on the device and registered on both contexts"""
    pk3 = filled(KEYS, 32)
    reserved.sig_keygen_dev(to_dev(sk3), pk3, KEYS)
    reserved.sync()
    for e in (fresh, reserved):
        assert not e.keyset_set(host(pk3)).any()
    return host(pk3)


def spoiled_steps(honest, byte, bit):
    """honest: one array of signatures or proofs per step.  Per step: a copy on the device with one byte of the middle row changed, and that row"""
    out = []
    for good in honest:
        bad, row = good.copy(), len(good) // 2
        bad[row, byte] ^= bit
        out.append((to_dev(bad), row))
    return out


def check_verdicts(ok, status, bad_row):
    want = np.ones(len(ok), dtype=np.uint8)
    want[bad_row] = 0
    assert np.array_equal(ok, want) and not status.any(), (len(ok), bad_row, ok.tolist(), status.tolist())


def run_both(fresh, reserved, enqueue):
    """enqueue(engine, sync_each) -> list of output tensors.  The fresh context runs with one synchronisation at the end, the reserved one with
    one after every call; returns the fresh context's outputs as arrays, after checking them byte-equal to the reserved context's."""
    import torch
    torch.cuda.synchronize()                    # the inputs and the pre-filled outputs are in place before either context's stream starts
    got = enqueue(fresh, lambda: None)
    fresh.sync()
    want = enqueue(reserved, reserved.sync)
    reserved.sync()
    got, want = [host(t) for t in got], [host(t) for t in want]
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), [i for i, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]
    return got


def test_signature_checks_nested_two_and_three_deep(pair):
    fresh, reserved = pair
    ids, sk3, matrix, lens, scalars = rows(9001)
    pk3 = registered(fresh, reserved, sk3)
    d_sk, d_pk, d_ids, d_m, d_len = to_dev(sk3[ids]), to_dev(pk3[ids]), to_dev(ids), to_dev(matrix), to_dev(lens)
    d_k, d_l = to_dev(scalars[0]), to_dev(scalars[1])
    sigs = filled(TOP, 64)
    reserved.sig_sign_dev(d_sk, d_pk, d_m, STRIDE, d_len, 0, sigs, TOP)
    reserved.sync()
    spoiled = spoiled_steps([host(sigs)[:n] for n in STEPS], 40, 1)

    def enqueue(e, after):
        outs = []
        for n, (bad, _) in zip(STEPS, spoiled):
            ok, st, ok_k, st_k, out, st_d = filled(n), filled(n), filled(n), filled(n), filled(n, 32), filled(n)
            e.sig_verify_dev(d_pk, d_m, STRIDE, d_len, 0, bad, ok, st, n); after()
            e.sig_verify_keyed_dev(d_ids, d_m, STRIDE, d_len, 0, bad, ok_k, st_k, n); after()
            e.keyset_double_mul_bytes_dev(d_k, d_l, d_ids, out, st_d, n); after()
            outs += [ok, st, ok_k, st_k, out, st_d]
        return outs
    got = run_both(fresh, reserved, enqueue)
    for step, (_, bad_row) in enumerate(spoiled):
        ok, st, ok_k, st_k, out, st_d = got[6 * step:6 * step + 6]
        check_verdicts(ok, st, bad_row)
        check_verdicts(ok_k, st_k, bad_row)
        assert not st_d.any() and out.any(axis=1).all()


def honest_elements(reserved, seed):
    """TOP blinded elements and their evaluations under one key, made on the device: (key words, blinded, evaluated)"""
    rng = np.random.default_rng(seed)
    key = rng.integers(1, 1 << 63, size=4, dtype=np.uint64)
    matrix, lens = rng.integers(0, 256, size=(TOP, STRIDE), dtype=np.uint8), rng.integers(0, STRIDE + 1, size=TOP).astype(np.uint32)
    blinds = rng.integers(1, 1 << 63, size=(TOP, 4), dtype=np.uint64)
    blinded, evaluated, st_b, st_e = filled(TOP, 32), filled(TOP, 32), filled(TOP), filled(TOP)
    reserved.oprf_blind_dev(to_dev(matrix), STRIDE, to_dev(lens), 0, to_dev(blinds), blinded, st_b, TOP, dst=DST)
    reserved.oprf_evaluate_dev(key, blinded, evaluated, st_e, TOP)
    reserved.sync()
    assert not host(st_b).any() and not host(st_e).any()
    return key, blinded, evaluated


def test_oprf_evaluate_over_the_dh_call(pair):
    fresh, reserved = pair
    key, blinded, evaluated = honest_elements(reserved, 9002)

    def enqueue(e, after):
        outs = []
        for n in STEPS:
            out, st = filled(n, 32), filled(n)
            e.oprf_evaluate_dev(key, blinded, out, st, n); after()
            outs += [out, st]
        return outs
    got = run_both(fresh, reserved, enqueue)
    for step, n in enumerate(STEPS):
        assert np.array_equal(got[2 * step], host(evaluated)[:n]) and not got[2 * step + 1].any()


def test_dleq_prove_then_verify(pair):
    fresh, reserved = pair
    key, blinded, evaluated = honest_elements(reserved, 9003)
    pk32 = reserved.dleq_public_key(key).tobytes()
    nonces = to_dev(np.random.default_rng(9004).integers(1, 1 << 63, size=(DLEQ_SHAPES[-1][0], 4), dtype=np.uint64))
    honest = []
    for groups, group_size in DLEQ_SHAPES:
        proofs, st = filled(groups, 64), filled(groups)
        reserved.dleq_prove_dev(key, blinded, evaluated, nonces, proofs, st, groups, group_size, dst=DST)
        reserved.sync()
        assert not host(st).any()
        honest.append(host(proofs))
    spoiled = spoiled_steps(honest, 3, 4)

    def enqueue(e, after):
        outs = []
        for (groups, group_size), (bad, _) in zip(DLEQ_SHAPES, spoiled):
            proofs, st_p, ok, st_v = filled(groups, 64), filled(groups), filled(groups), filled(groups)
            e.dleq_prove_dev(key, blinded, evaluated, nonces, proofs, st_p, groups, group_size, dst=DST); after()
            e.dleq_verify_dev(pk32, blinded, evaluated, bad, ok, st_v, groups, group_size, dst=DST); after()
            outs += [proofs, st_p, ok, st_v]
        return outs
    got = run_both(fresh, reserved, enqueue)
    for step, (_, bad_group) in enumerate(spoiled):
        proofs, st_p, ok, st_v = got[4 * step:4 * step + 4]
        assert np.array_equal(proofs, honest[step]) and not st_p.any()
        check_verdicts(ok, st_v, bad_group)


def test_vrf_prove_then_verify_and_keyed_verify(pair):
    fresh, reserved = pair
    ids, sk3, matrix, lens, _ = rows(9005)
    pk3 = registered(fresh, reserved, sk3)
    d_sk, d_pk, d_ids, d_m, d_len = to_dev(sk3[ids]), to_dev(pk3[ids]), to_dev(ids), to_dev(matrix), to_dev(lens)
    honest = filled(TOP, 96)
    reserved.vrf_prove_dev(d_sk, d_pk, d_m, STRIDE, d_len, 0, honest, TOP, dst=DST)
    reserved.sync()
    honest = host(honest)
    spoiled = spoiled_steps([honest[:n] for n in STEPS], 70, 2)

    def enqueue(e, after):
        outs = []
        for n, (bad, _) in zip(STEPS, spoiled):
            proofs, beta, ok, st, beta_k, ok_k, st_k = filled(n, 96), filled(n, 64), filled(n), filled(n), filled(n, 64), filled(n), filled(n)
            e.vrf_prove_dev(d_sk, d_pk, d_m, STRIDE, d_len, 0, proofs, n, dst=DST); after()
            e.vrf_verify_dev(d_pk, d_m, STRIDE, d_len, 0, bad, beta, ok, st, n, dst=DST); after()
            e.vrf_verify_keyed_dev(d_ids, d_m, STRIDE, d_len, 0, bad, beta_k, ok_k, st_k, n, dst=DST); after()
            outs += [proofs, beta, ok, st, beta_k, ok_k, st_k]
        return outs
    got = run_both(fresh, reserved, enqueue)
    for step, (n, (_, bad_row)) in enumerate(zip(STEPS, spoiled)):
        proofs, beta, ok, st, beta_k, ok_k, st_k = got[7 * step:7 * step + 7]
        assert np.array_equal(proofs, honest[:n])
        check_verdicts(ok, st, bad_row)
        check_verdicts(ok_k, st_k, bad_row)
        assert np.array_equal(beta, beta_k) and not beta[bad_row].any() and np.delete(beta, bad_row, axis=0).any(axis=1).all()


def test_grouped_host_arrays_after_another_user_grew_the_staging_buffer(pair):
    """fp2_mul of 70 000 rows stages 6.7 MB; msm_bytes over host arrays at (2, 65) then holds a staging buffer that another user has grown"""
    fresh, reserved = pair
    rng = np.random.default_rng(9006)
    groups, group_size = 2, 65
    n = groups * group_size
    scalars = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    points32 = reserved.encode(reserved.comb_mul(rng.integers(1, 1 << 63, size=(n, 4), dtype=np.uint64), _comb[0])[0])
    want, want_st = reserved.msm_bytes(scalars, points32, group_size)
    x = rng.integers(0, 1 << 62, size=(70000, 8), dtype=np.uint64)
    product = fresh.prim("FP2_MUL", x)
    got, got_st = fresh.msm_bytes(scalars, points32, group_size)
    assert np.array_equal(got, want) and np.array_equal(got_st, want_st) and not got_st.any() and got.shape == (groups, 32)
    assert np.array_equal(product[:1000], reserved.prim("FP2_MUL", x[:1000]))
