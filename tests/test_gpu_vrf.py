"""The verifiable random function on the device (fourq_vrf_*): prove, verify, the keyed verify and proof_to_hash against the fixture made
with the reference's point functions (tests/golden/vrf.json) and against the CPU restatement (tests/vrf_ref.py), whose answers are computed
once per process.  Every test takes `eng`: table selection by address and constant-time selection must agree bit for bit."""
import ctypes

import numpy as np
import pytest

import adversarial_points
import keyset_ref
import sig_ref
import vrf_ref as ref
from fourq_amd import _lib, codec
from test_gpu_sig import bad_rows, byte_rows, g_comb, to_dev

pytestmark = pytest.mark.gpu

N = ref.N
ROWS = 257
STRIDE = 203                                # no multiple of 8: rows are read by bytes
DST = b"FourQ-VRF-V01-gpu-tests"
NOT_ON_CURVE, RESERVED, REF_ATTRIBUTE = bytes([2] + [0] * 31), bytes([0] * 15 + [0x80] + [0] * 16), ref.NEUTRAL32
_cache = {}


def message_matrix(alphas, stride):
    matrix = np.zeros((len(alphas), stride), dtype=np.uint8)
    for i, a in enumerate(alphas):
        matrix[i, :len(a)] = np.frombuffer(a, dtype=np.uint8)
    return matrix, np.array([len(a) for a in alphas], dtype=np.uint32)


def batch():
    """ROWS honest rows, the restatement's: distinct keys, ragged alphas of 0..200 bytes in a matrix of STRIDE bytes per row; per process"""
    if "batch" not in _cache:
        rng = np.random.default_rng(8100)
        sks = [r.tobytes() for r in rng.integers(0, 256, size=(ROWS, 32), dtype=np.uint8)]
        pks = [sig_ref.keygen(sk) for sk in sks]
        lengths = [0, 1, 2, 31, 32, 33, 95, 96, 97, 127, 128, 200]
        alphas = [rng.integers(0, 256, size=lengths[i % len(lengths)] if i % 5 else int(rng.integers(0, 201)), dtype=np.uint8).tobytes() for i in range(ROWS)]
        proofs = [ref.prove(sk, pk, a, DST) for sk, pk, a in zip(sks, pks, alphas)]
        betas = [ref.proof_to_hash(p, DST) for p in proofs]
        assert all(st == 0 for _, st in betas) and ref.verify(pks[5], alphas[5], proofs[5], DST) == (1, 0, betas[5][0])
        matrix, lens = message_matrix(alphas, STRIDE)
        _cache["batch"] = dict(sks=byte_rows(sks, 32), pks=byte_rows(pks, 32), alphas=alphas, matrix=matrix, lens=lens, proofs=byte_rows(proofs, 96),
                               betas=byte_rows([b for b, _ in betas], 64))
    return _cache["batch"]


def dev_buffers(n):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.full((n, 64), 7, dtype=torch.uint8, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev))


def dev_verify(eng, keys, matrix, lens, proofs, dst=DST, keyed=False):
    n = len(proofs)
    beta, ok, st = dev_buffers(n)
    call = eng.vrf_verify_keyed_dev if keyed else eng.vrf_verify_dev
    call(to_dev(keys), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, to_dev(proofs), beta, ok, st, n, dst=dst)
    eng.sync()
    return beta.cpu().numpy(), ok.cpu().numpy(), st.cpu().numpy()


def expect(rows):
    """(beta, ok, status) arrays of a list of the restatement's (ok, status, beta) rows"""
    return byte_rows([r[2] for r in rows], 64), np.array([r[0] for r in rows], dtype=np.uint8), np.array([r[1] for r in rows], dtype=np.uint8)


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 1. rows computed with the real reference's point functions ------------------------------------------------------------------
def test_fixture_bit_exact(eng, golden):
    import torch
    rows = golden("vrf.json", raw=True)["rows"]
    comb = g_comb(eng)
    for dst in sorted({r["dst"] for r in rows}):
        under = [r for r in rows if r["dst"] == dst]
        dst = bytes.fromhex(dst)
        col = lambda key, width: byte_rows([bytes.fromhex(r[key]) for r in under], width)
        sk, pk, proof, beta = col("sk", 32), col("pk", 32), col("proof", 96), col("beta", 64)
        honest = byte_rows([bytes.fromhex(r.get("honest_proof", r["proof"])) for r in under], 96)
        matrix, lens = codec.pack_messages([bytes.fromhex(r["alpha"]) for r in under])
        got = eng.vrf_prove(sk, pk, matrix, lens, dst=dst, comb=comb)
        assert bad_rows(got, honest).size == 0, [under[i]["kind"] for i in bad_rows(got, honest)]
        out = torch.full((len(under), 96), 7, dtype=torch.uint8, device=torch.device("cuda", 0))
        eng.vrf_prove_dev(to_dev(sk), to_dev(pk), to_dev(matrix), matrix.shape[1], to_dev(lens), 0, out, len(under), dst=dst)
        eng.sync()
        assert bad_rows(out.cpu().numpy(), honest).size == 0
        want = (beta, np.ones(len(under), dtype=np.uint8), np.zeros(len(under), dtype=np.uint8))
        assert same(eng.vrf_verify(pk, matrix, proof, lens, dst=dst, comb=comb), want)          # the torsion-shifted rows among them
        assert same(dev_verify(eng, pk, matrix, lens, proof, dst), want)
        assert same(eng.vrf_proof_to_hash(proof, dst=dst), (beta, want[2]))
        assert same(eng.vrf_proof_to_hash(honest, dst=dst), (beta, want[2]))


# ---- 2. shapes: a lane, a wave edge, a block edge; the sum of two has 2 n rows on either side of the same edges ---------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_shapes_against_the_restatement(eng, n):
    b = batch()
    comb = g_comb(eng)
    assert b["matrix"].shape[1] % 8 != 0 and b["lens"].max() == 200 and b["lens"].min() == 0 and len({r.tobytes() for r in b["pks"]}) == ROWS
    got = eng.vrf_prove(b["sks"][:n], b["pks"][:n], b["matrix"][:n], b["lens"][:n], dst=DST, comb=comb)
    assert bad_rows(got, b["proofs"][:n]).size == 0, bad_rows(got, b["proofs"][:n])
    want = (b["betas"][:n], np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8))
    assert same(eng.vrf_verify(b["pks"][:n], b["matrix"][:n], got, b["lens"][:n], dst=DST, comb=comb), want)
    assert same(dev_verify(eng, b["pks"][:n], b["matrix"][:n], b["lens"][:n], got), want)
    assert same(eng.vrf_proof_to_hash(got, dst=DST), (want[0], want[2]))


# ---- 3. soundness: every tampering fails exactly its own rows ------------------------------------------------------------------------
def test_soundness_exactly_the_listed_rows_fail(eng):
    b = batch()
    comb = g_comb(eng)
    n = 65
    pks, proofs = [r.tobytes() for r in b["pks"][:n]], [r.tobytes() for r in b["proofs"][:n]]
    labels = []
    for label, pk_t, a_t, p_t, dst_t, failing in ref.soundness_cases(pks, b["alphas"][:n], proofs, DST):
        matrix, lens = message_matrix(a_t, STRIDE)
        beta, ok, st = eng.vrf_verify(byte_rows(pk_t, 32), matrix, byte_rows(p_t, 96), lens, dst=dst_t, comb=comb)
        want_ok = np.ones(n, dtype=np.uint8)
        want_ok[failing] = 0
        want_beta = b["betas"][:n].copy()
        want_beta[failing] = 0
        assert np.array_equal(ok, want_ok) and not st.any() and bad_rows(beta, want_beta).size == 0, label
        labels.append(label)
    assert len(labels) == 8


# ---- 4. statuses: one batch with one row of each kind, honest rows next to them --------------------------------------------------------
def status_batch():
    b = batch()
    n = 40
    pks, proofs = [r.tobytes() for r in b["pks"][:n]], [r.tobytes() for r in b["proofs"][:n]]
    n_row = N.to_bytes(32, "little")
    order7 = next(adversarial_points.encode(T) for label, T in adversarial_points.torsion()
                  if label.startswith("seeded torsion") and adversarial_points.order_in_392(T) == 7)
    kinds = {}
    for at, bad in ((1, RESERVED), (4, NOT_ON_CURVE), (7, REF_ATTRIBUTE)):
        pks[at] = bad
        kinds[at] = sig_ref.decode_status(bad)[0]
    proofs[10] = NOT_ON_CURVE + proofs[10][32:]; kinds[10] = 16 + 2
    proofs[13] = proofs[13][:32] + n_row + proofs[13][64:]; kinds[13] = ref.SIG_S_RANGE
    proofs[16] = proofs[16][:64] + n_row; kinds[16] = ref.SIG_S_RANGE
    proofs[19] = order7 + proofs[19][32:]; kinds[19] = ref.GAMMA_NEUTRAL
    proofs[22] = RESERVED + n_row + n_row; kinds[22] = 16 + 1                         # undecodable and out of range: the decode code wins
    pks[25] = NOT_ON_CURVE; proofs[25] = RESERVED + proofs[25][32:]; kinds[25] = 16 + 2  # the key before Gamma
    proofs[28] = order7 + n_row + proofs[28][64:]; kinds[28] = ref.SIG_S_RANGE          # the range before the neutral W
    return b, n, pks, proofs, kinds


def test_statuses_and_their_precedence(eng):
    b, n, pks, proofs, kinds = status_batch()
    comb = g_comb(eng)
    want = expect([ref.verify(pk, a, p, DST) for pk, a, p in zip(pks, b["alphas"][:n], proofs)])
    assert {i: int(want[2][i]) for i in np.flatnonzero(want[2])} == kinds
    assert want[1].sum() == n - len(kinds) and not want[0][want[1] == 0].any() and bad_rows(want[0][want[1] == 1], b["betas"][:n][want[1] == 1]).size == 0
    pk_rows, proof_rows = byte_rows(pks, 32), byte_rows(proofs, 96)
    assert same(eng.vrf_verify(pk_rows, b["matrix"][:n], proof_rows, b["lens"][:n], dst=DST, comb=comb), want)
    assert same(dev_verify(eng, pk_rows, b["matrix"][:n], b["lens"][:n], proof_rows), want)
    p2h = [ref.proof_to_hash(p, DST) for p in proofs]
    assert same(eng.vrf_proof_to_hash(proof_rows, dst=DST), (byte_rows([x[0] for x in p2h], 64), np.array([x[1] for x in p2h], dtype=np.uint8)))
    assert {x[1] for x in p2h} == {0, 16 + 1, 16 + 2, ref.GAMMA_NEUTRAL}
    # _dev: a length above the stride is clamped and reported -- behind a decode code, in front of the range
    over = b["lens"][:n].copy()
    over[[2, 4, 13]] = STRIDE + 1
    beta, ok, st = dev_verify(eng, pk_rows, b["matrix"][:n], over, proof_rows)
    clamped = want[2].copy()
    clamped[[2, 13]] = _lib.SIG_MSG_CLAMPED
    assert np.array_equal(st, clamped) and np.array_equal(ok, (clamped == 0).astype(np.uint8)) and not beta[clamped != 0].any()
    assert bad_rows(beta[clamped == 0], want[0][clamped == 0]).size == 0


# ---- 5. a Gamma shifted by torsion: accepted, with the honest row's beta ----------------------------------------------------------------
def test_torsion_shifted_gamma_keeps_the_honest_beta(eng):
    b = batch()
    comb = g_comb(eng)
    torsion = {}
    for label, T in adversarial_points.torsion():
        if label.startswith("seeded torsion"):
            torsion.setdefault(adversarial_points.order_in_392(T), T)
    n = 6
    orders = [7, 14, 28, 7, 14, 56]
    shifted = [ref.prove(b["sks"][i].tobytes(), b["pks"][i].tobytes(), b["alphas"][i], DST, shift=torsion[orders[i]]) for i in range(n)]
    assert all(s[:32] != b["proofs"][i].tobytes()[:32] for i, s in enumerate(shifted))
    want = (b["betas"][:n], np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8))
    assert same(eng.vrf_verify(b["pks"][:n], b["matrix"][:n], byte_rows(shifted, 96), b["lens"][:n], dst=DST, comb=comb), want)
    assert same(eng.vrf_proof_to_hash(byte_rows(shifted, 96), dst=DST), (want[0], want[2]))


# ---- 6. registered keys -------------------------------------------------------------------------------------------------------------------
def test_keyed_verify_equals_the_unkeyed_call_on_the_keys_of_the_rows(eng):
    from fourq_amd import FourQError
    b = batch()
    comb = g_comb(eng)
    A = sig_ref.decode_status(b["pks"][1].tobytes())[1]
    p = ref.o.P127
    order_2n = adversarial_points.encode((tuple((-c) % p for c in A[0]), tuple((-c) % p for c in A[1])))
    slots = [0, None, 2, None, 4]                 # slot -> batch key; slot 1 is (-x, -y) of an honest key, slot 3 does not decode
    keys = np.stack([b["pks"][0], np.frombuffer(order_2n, dtype=np.uint8), b["pks"][2], np.frombuffer(NOT_ON_CURVE, dtype=np.uint8), b["pks"][4]])
    key_st = [keyset_ref.key_status(k.tobytes()) for k in keys]
    assert key_st == [0, ref.KEYSET_NOT_ORDER_N, 0, 16 + 2, 0] and list(eng.keyset_set(keys)) == key_st
    n = 130
    ids = np.random.default_rng(8600).integers(0, 5, size=n).astype(np.uint32)
    ids[:5] = np.arange(5)
    if "keyed" not in _cache:
        owner = [slots[i] if slots[i] is not None else 0 for i in ids]
        alphas = [b["alphas"][i % ROWS] for i in range(n)]
        proofs = [ref.prove(b["sks"][j].tobytes(), b["pks"][j].tobytes(), a, DST) for j, a in zip(owner, alphas)]
        for i in range(7, n, 9):
            proofs[i] = proofs[i][:40] + bytes([proofs[i][40] ^ 1]) + proofs[i][41:]             # a few that do not hold
        _cache["keyed"] = (alphas, proofs)
    alphas, proofs = _cache["keyed"]
    matrix, lens = message_matrix(alphas, STRIDE)
    proof_rows = byte_rows(proofs, 96)
    unkeyed = eng.vrf_verify(keys[ids], matrix, proof_rows, lens, dst=DST, comb=comb)
    accepted = np.array([key_st[i] == 0 for i in ids])
    want_st = np.where(accepted, unkeyed[2], np.array(key_st, dtype=np.uint8)[ids]).astype(np.uint8)
    want = (np.where(accepted[:, None], unkeyed[0], 0).astype(np.uint8), np.where(accepted, unkeyed[1], 0).astype(np.uint8), want_st)
    assert 0 < want[1].sum() < accepted.sum() and {0, ref.KEYSET_NOT_ORDER_N, 16 + 2} == set(want_st)
    assert want[1].sum() == accepted.sum() - len([i for i in range(7, n, 9) if accepted[i]])
    got = eng.vrf_verify_keyed(ids, matrix, proof_rows, lens, dst=DST, comb=comb)
    assert same(got, want)
    assert same(dev_verify(eng, ids, matrix, lens, proof_rows, keyed=True), want)
    # the restatement agrees, and so does the other selection mode (both modes run this test against the same expectations)
    assert same(got, expect([ref.verify_keyed([k.tobytes() for k in keys], int(i), a, pr, DST) for i, a, pr in zip(ids, alphas, proofs)]))
    # an index outside the set: the host flavour refuses the call, the _dev flavour clamps it and reports it
    far = ids.copy()
    far[3::11] = 5
    far[4::11] = 0xFFFFFFFF
    with pytest.raises(FourQError):
        eng.vrf_verify_keyed(far, matrix, proof_rows, lens, dst=DST, comb=comb)
    outside = far >= 5
    beta, ok, st = dev_verify(eng, far, matrix, lens, proof_rows, keyed=True)
    assert np.array_equal(st, np.where(outside, _lib.KEYSET_ID_RANGE, want[2])) and np.array_equal(ok, np.where(outside, 0, want[1]))
    assert bad_rows(beta, np.where(outside[:, None], 0, want[0])).size == 0


# ---- 7. the argument contract and the reservation -----------------------------------------------------------------------------------------
def test_argument_contract(eng):
    import torch
    from fourq_amd import Engine
    dev = torch.device("cuda", 0)
    b = batch()
    g_comb(eng)
    eng.keyset_set(b["pks"][:4])
    lib, ctx = eng._lib, eng._ctx
    n = 64
    buf = lambda nbytes: torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    sk, pk, ids, proof, beta, ok, st, msg = buf(32 * n), buf(32 * n), buf(4 * n), buf(96 * n), buf(64 * n), buf(n), buf(n), buf(16 * n)
    pk[:32 * n] = to_dev(b["pks"][:n].reshape(-1))
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    dst = ctypes.create_string_buffer(bytes(range(1, 256)) + b"\x01", 256)
    prove, verify, keyed, p2h = lib.fourq_vrf_prove_dev, lib.fourq_vrf_verify_dev, lib.fourq_vrf_verify_keyed_dev, lib.fourq_vrf_proof_to_hash_dev
    good_prove = [p(sk), p(pk), None, dst, 5, p(msg), 16, None, 16, p(proof)]
    good_verify = [p(pk), None, dst, 5, p(msg), 16, None, 16, p(proof), p(beta), p(ok), p(st)]
    good_keyed = [p(ids)] + good_verify[1:]
    good_p2h = [dst, 5, p(proof), p(beta), p(st)]
    calls = ((prove, good_prove, (0, 1, 9), ((0, sk), (1, pk), (9, proof))), (verify, good_verify, (0, 8, 9, 10, 11), ((0, pk), (8, proof), (9, beta))),
             (keyed, good_keyed, (0, 8, 9, 10, 11), ((0, ids), (8, proof), (9, beta))), (p2h, good_p2h, (2, 3, 4), ((2, proof), (3, beta))))
    for fn, good, arrays, aligned in calls:
        at_dst = good.index(dst)
        assert fn(ctx, *good, n) == _lib.OK and fn(None, *good, n) == _lib.ERR_INVALID
        for at in arrays:                                             # every array: NULL
            args = list(good); args[at] = None
            assert fn(ctx, *args, n) == _lib.ERR_INVALID, at
        for at, t in aligned:                                         # every _dev array but ok and status: misaligned
            args = list(good); args[at] = p(t, 8)
            assert fn(ctx, *args, n) == _lib.ERR_INVALID, at
        for bad_len in (0, 256):                                      # dst: 1..255 bytes
            args = list(good); args[at_dst + 1] = bad_len
            assert fn(ctx, *args, n) == _lib.ERR_INVALID
        args = list(good); args[at_dst] = None
        assert fn(ctx, *args, n) == _lib.ERR_INVALID
        args = list(good); args[at_dst + 1] = 255
        assert fn(ctx, *args, n) == _lib.OK
        assert fn(ctx, *good, _lib.MAX_BATCH + 1) == _lib.ERR_INVALID
    assert verify(ctx, *good_verify, _lib.MAX_BATCH // 2 + 1) == _lib.ERR_INVALID         # the sum of two has 2 n rows
    args = list(good_verify); args[10] = p(ok, 1); args[11] = p(st, 3)                   # ok and status need not be aligned
    assert verify(ctx, *args, n) == _lib.OK
    eng.sync()
    for t in (proof, beta, ok, st):
        t.fill_(9)
    for fn, good, _, _ in calls:                                      # n == 0: OK, nothing touched
        assert fn(ctx, *good, 0) == _lib.OK
    eng.sync()
    assert all((t.cpu().numpy() == 9).all() for t in (proof, beta, ok, st))
    assert lib.fourq_vrf_reserve(ctx, _lib.MAX_BATCH // 2 + 1) == _lib.ERR_INVALID and lib.fourq_vrf_reserve(ctx, 0) == _lib.OK
    assert lib.fourq_vrf_reserve(None, 1) == _lib.ERR_INVALID
    with Engine(0) as e:                                              # the keyed call with no set installed
        e.ct_select = eng.ct_select
        e.comb_stage(e.comb_table(codec.pack_point(sig_ref.G1)))
        assert e._lib.fourq_vrf_verify_keyed_dev(e._ctx, *good_keyed, n) == _lib.ERR_INVALID
        assert e._lib.fourq_vrf_verify_keyed_dev(e._ctx, *good_keyed, 0) == _lib.OK


def test_two_unsynchronised_dev_verifies_after_a_reservation(eng):
    from fourq_amd import Engine
    b = batch()
    n1, n2 = 100, 157
    spoiled = b["proofs"].copy()
    spoiled[n1 + 3::10, 70] ^= 2
    want2 = np.ones(n2, dtype=np.uint8)
    want2[3::10] = 0
    with Engine(0) as e:
        e.ct_select = eng.ct_select
        e.comb_stage(e.comb_table(codec.pack_point(sig_ref.G1)))
        e.vrf_reserve(n2)
        d_pk, d_m, d_len, d_p = to_dev(b["pks"]), to_dev(b["matrix"]), to_dev(b["lens"]), to_dev(spoiled)
        beta1, ok1, st1 = dev_buffers(n1)
        beta2, ok2, st2 = dev_buffers(n2)
        second = lambda t, width: t.view(-1)[n1 * width:]
        e.vrf_verify_dev(d_pk, d_m, STRIDE, d_len, 0, d_p, beta1, ok1, st1, n1, dst=DST)
        # the second call starts at row n1: 16-byte aligned slices of the same arrays (n1 is a multiple of 4), and a matrix of its own
        pk2, p2, len2 = second(d_pk, 32), second(d_p, 96), d_len[n1:]
        m2 = to_dev(b["matrix"][n1:])
        e.vrf_verify_dev(pk2, m2, STRIDE, len2, 0, p2, beta2, ok2, st2, n2, dst=DST)
        e.sync()
        assert ok1.cpu().numpy().all() and not st1.cpu().numpy().any() and bad_rows(beta1.cpu().numpy(), b["betas"][:n1]).size == 0
        assert np.array_equal(ok2.cpu().numpy(), want2) and not st2.cpu().numpy().any()
        want_beta = b["betas"][n1:].copy()
        want_beta[want2 == 0] = 0
        assert bad_rows(beta2.cpu().numpy(), want_beta).size == 0


# ---- 8. the module on bytes -------------------------------------------------------------------------------------------------------------------
def test_bytes_module_round_trip_and_known_answer():
    from fourq_amd import schnorrq, vrf
    sk, alpha = bytes.fromhex(vrf.KAT_SK), bytes.fromhex(vrf.KAT_ALPHA)
    pk = schnorrq.keygen(sk)
    assert pk.hex() == vrf.KAT_PK
    proof = vrf.prove(sk, alpha, vrf.KAT_DST)
    assert proof.hex() == vrf.KAT_PROOF and vrf.prove(sk, alpha, vrf.KAT_DST, pk) == proof
    beta = vrf.verify(pk, alpha, proof, vrf.KAT_DST)
    assert beta.hex() == vrf.KAT_BETA and vrf.proof_to_hash(proof, vrf.KAT_DST) == beta
    assert vrf.verify(pk, alpha + b"!", proof, vrf.KAT_DST) is None and vrf.verify(pk, alpha, proof, vrf.KAT_DST + b"2") is None
    b = batch()
    sks, pks = [r.tobytes() for r in b["sks"][:5]], [r.tobytes() for r in b["pks"][:5]]
    proofs = vrf.prove_many(sks, b["alphas"][:5], DST)
    assert proofs == [r.tobytes() for r in b["proofs"][:5]]
    assert vrf.verify_many(pks, b["alphas"][:5], proofs, DST) == [r.tobytes() for r in b["betas"][:5]] == vrf.proof_to_hash_many(proofs, DST)
    with pytest.raises(ValueError):
        vrf.verify(NOT_ON_CURVE, alpha, proof, vrf.KAT_DST)
    with pytest.raises(ValueError):
        vrf.proof_to_hash(NOT_ON_CURVE + proof[32:], vrf.KAT_DST)
    assert vrf.prove_many([], [], DST) == [] and vrf.verify_many([], [], [], DST) == []


# ---- 9. several devices -------------------------------------------------------------------------------------------------------------------
def test_multi_engine_equals_engine(eng):
    import torch
    from fourq_amd import MultiEngine
    b = batch()
    comb = g_comb(eng)
    n = ROWS
    proofs = b["proofs"].copy()
    proofs[5::17, 40] ^= 4
    keys = b["pks"][:8]
    ids = (np.arange(n) % 8).astype(np.uint32)
    eng.keyset_set(keys)
    want = (eng.vrf_prove(b["sks"], b["pks"], b["matrix"], b["lens"], dst=DST, comb=comb),) + eng.vrf_verify(b["pks"], b["matrix"], proofs, b["lens"], dst=DST, comb=comb) + \
        eng.vrf_verify_keyed(ids, b["matrix"], proofs, b["lens"], dst=DST, comb=comb) + eng.vrf_proof_to_hash(proofs, dst=DST)
    devices = list(range(torch.cuda.device_count())) if torch.cuda.device_count() > 1 else [0, 0]
    with MultiEngine(devices) as multi:
        multi.ct_select = eng.ct_select
        multi.keyset_set(keys)
        got = (multi.vrf_prove(b["sks"], b["pks"], b["matrix"], b["lens"], dst=DST, comb=comb),) + multi.vrf_verify(b["pks"], b["matrix"], proofs, b["lens"], dst=DST, comb=comb) + \
            multi.vrf_verify_keyed(ids, b["matrix"], proofs, b["lens"], dst=DST, comb=comb) + multi.vrf_proof_to_hash(proofs, dst=DST)
    assert len(got) == len(want) == 9 and same(got, want)
    assert bad_rows(want[0], b["proofs"]).size == 0 and want[2].sum() == n - len(range(5, n, 17)) and 0 < want[5].sum() < n
