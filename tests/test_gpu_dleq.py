"""The batched DLEQ proofs on the device (fourq_dleq_*, dleq.hip.h) against the fixture tests/golden/dleq.json and the CPU restatement
tests/dleq_ref.py, in both selection modes.  The restatement's answers are computed once per process and shared by both engines; the rows
of the larger shapes are an arithmetic progression P_0 + i Q in the subgroup of order N, so that the server's evaluation of every row is
an addition on the CPU ([K](P_0 + i Q) = [K]P_0 + i [K]Q; the first rows are checked against DH_endo itself)."""
import functools
import random

import numpy as np
import pytest

import curve4q_oracle as o
import dleq_ref as ref
import oprf_ref
from conftest import load_golden
from fourq_amd import FourQError, _lib, codec

pytestmark = pytest.mark.gpu
N = ref.N
DST = b"FourQ-DLEQ-V01-test"
SHAPES = ((1, 1), (1, 2), (3, 5), (257, 1), (2, 65), (5, 64), (1, 257))       # (groups, group_size)
POOL = 320
NOT_ON_CURVE = bytes([2] + [0] * 31)
G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
_combs = {}


def rows_of(items, width):
    return np.frombuffer(b"".join(bytes(b) for b in items), dtype=np.uint8).reshape(len(items), width).copy()


def staged(eng):
    """the engine with the generator's comb staged: the dleq calls below pass comb = None"""
    if id(eng) not in _combs:
        _combs[id(eng)] = eng.comb_table(G1_WORDS)
        eng.comb_stage(_combs[id(eng)])
    return eng


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


def dev_full(shape, value=0xAA):
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=torch.uint8, device=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def pool():
    """key, pk32 and POOL honest rows (blinded, evaluated) as lists of 32 bytes"""
    rng = random.Random(20261019)
    key = rng.getrandbits(256)
    pk32, st = ref.public_key(key)
    assert st == 0
    aff = lambda m: o.R1toAffine(o.MUL_endo(m, o.AffineToR1(o.Gx, o.Gy)))
    P0, Q = aff(rng.randrange(1, N)), aff(rng.randrange(1, N))
    step = lambda A, B: o.R1toAffine(o.ADD(o.AffineToR1(A[0], A[1]), o.R1toR2(o.AffineToR1(B[0], B[1]))))
    D0, DQ = o.DH_endo(key, P0), o.DH_endo(key, Q)
    blinded, evaluated = [], []
    for _ in range(POOL):
        blinded.append(ref.enc(P0))
        evaluated.append(ref.enc(D0))
        P0, D0 = step(P0, Q), step(D0, DQ)
    assert all(oprf_ref.evaluate(key, blinded[i]) == (evaluated[i], 0) for i in (0, 1, 2, POOL - 1))
    return key, pk32, blinded, evaluated


@functools.lru_cache(maxsize=None)
def shape(groups, group_size):
    """the restatement's answers for the first groups x group_size rows of the pool: nonces, proofs, M32 and Z32 per group"""
    key, pk32, blinded, evaluated = pool()
    n = groups * group_size
    rng = random.Random(groups * 1000 + group_size)
    nonces = [rng.getrandbits(256) for _ in range(groups)]
    proofs, m32, z32 = [], [], []
    for g in range(groups):
        cs, ds = blinded[g * group_size:(g + 1) * group_size], evaluated[g * group_size:(g + 1) * group_size]
        proof, st, parts = ref.prove_group(key, cs, ds, nonces[g], DST, parts=True)
        assert st == 0
        proofs.append(proof), m32.append(parts["M32"]), z32.append(parts["Z32"])
    first = ref.verify_group(pk32, blinded[:group_size], evaluated[:group_size], proofs[0], DST)
    assert first == (1, 0)                                          # ... and the prover's Z32 is the verifier's: checked on the device below for every group
    return {"n": n, "k": codec.pack_scalars([key])[0], "pk": pk32, "b": rows_of(blinded[:n], 32), "e": rows_of(evaluated[:n], 32), "r": codec.pack_scalars(nonces),
            "proofs": rows_of(proofs, 64), "m32": rows_of(m32, 32), "z32": rows_of(z32, 32)}


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------
def test_fixture_groups_are_bit_exact(eng):
    staged(eng)
    cases = load_golden("dleq.json", raw=True)["cases"]
    assert len(cases) >= 20
    for c in cases:
        dst, key, pk, gs = bytes.fromhex(c["dst"]), int(c["key"], 16), bytes.fromhex(c["pk"]), c["group_size"]
        b = rows_of([bytes.fromhex(x) for g in c["groups"] for x in g["blinded"]], 32)
        e = rows_of([bytes.fromhex(x) for g in c["groups"] for x in g["evaluated"]], 32)
        k, r = codec.pack_scalars([key])[0], codec.pack_scalars([int(g["nonce"], 16) for g in c["groups"]])
        want = rows_of([bytes.fromhex(g["proof"]) for g in c["groups"]], 64)
        label = (len(dst), gs)
        assert eng.dleq_public_key(k).tobytes() == pk, label
        m32, z32, st = eng.dleq_composites(pk, b, e, gs, dst=dst)
        assert not st.any() and [x.tobytes().hex() for x in m32] == [g["M32"] for g in c["groups"]] and [x.tobytes().hex() for x in z32] == [g["Z32"] for g in c["groups"]], label
        proofs, st = eng.dleq_prove(k, b, e, r, gs, dst=dst)
        assert not st.any() and np.array_equal(proofs, want), label
        ok, st = eng.dleq_verify(pk, b, e, want, gs, dst=dst)
        assert not st.any() and ok.all(), label


# ---- 2. shapes: a lane, a block and a fold pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups,group_size", SHAPES)
def test_shapes_against_the_restatement(eng, groups, group_size):
    staged(eng)
    s = shape(groups, group_size)
    m32, z32, st = eng.dleq_composites(s["pk"], s["b"], s["e"], group_size, dst=DST)
    assert not st.any() and np.array_equal(m32, s["m32"]) and np.array_equal(z32, s["z32"])       # d through the sums; the verifier's Z is the prover's
    proofs, st = eng.dleq_prove(s["k"], s["b"], s["e"], s["r"], group_size, dst=DST)
    assert not st.any() and np.array_equal(proofs, s["proofs"])
    ok, st = eng.dleq_verify(s["pk"], s["b"], s["e"], proofs, group_size, dst=DST)
    assert not st.any() and ok.all() and len(ok) == groups


# ---- 3. soundness -----------------------------------------------------------------------------------------------------------------------------
def test_every_tampering_fails_its_group_and_only_its_group(eng):
    staged(eng)
    key, pk32, blinded, evaluated = pool()
    groups, gs = 4, 3
    b, e = blinded[:groups * gs], evaluated[:groups * gs]
    proofs, st = eng.dleq_prove(codec.pack_scalars([key])[0], rows_of(b, 32), rows_of(e, 32), codec.pack_scalars([5, 6, 7, 8]), gs, dst=DST)     # pinned by the tests above
    assert not st.any()
    labels = 0
    for label, pk_t, bt, et, pt, dst_t, failing in ref.soundness_cases(key, pk32, b, e, [p.tobytes() for p in proofs], DST, gs):
        ok, st = eng.dleq_verify(pk_t, rows_of(bt, 32), rows_of(et, 32), rows_of(pt, 64), gs, dst=dst_t)
        assert not st.any() and ok.tolist() == [0 if g in failing else 1 for g in range(groups)], label
        labels += 1
    assert labels == 7
    # s + N is another encoding of the same residue: out of range, and only that group
    second = proofs.copy()
    sN = int.from_bytes(second[2, 32:].tobytes(), "little") + N
    second[2, 32:] = np.frombuffer(sN.to_bytes(32, "little"), dtype=np.uint8)
    ok, st = eng.dleq_verify(pk32, rows_of(b, 32), rows_of(e, 32), second, gs, dst=DST)
    assert ok.tolist() == [1, 1, 0, 1] and st.tolist() == [0, 0, _lib.SIG_S_RANGE, 0]


# ---- 4. statuses: each code by one group among good ones ----------------------------------------------------------------------------------------
def test_statuses_mark_one_group_and_zero_its_row(eng):
    staged(eng)
    key, pk32, blinded, evaluated = pool()
    groups, gs = 4, 2
    n = groups * gs
    k, r = codec.pack_scalars([key])[0], codec.pack_scalars([11, 12, 13, 14])
    good_b, good_e = rows_of(blinded[:n], 32), rows_of(evaluated[:n], 32)
    good, st = eng.dleq_prove(k, good_b, good_e, r, gs, dst=DST)
    assert not st.any() and [(p.tobytes(), 0) for p in good] == ref.prove(key, blinded[:n], evaluated[:n], [11, 12, 13, 14], DST, gs)

    def check_prove(b, e, nonces, key_int, note):
        want = ref.prove(key_int, [x.tobytes() for x in b], [x.tobytes() for x in e], nonces, DST, gs)
        out, st = eng.dleq_prove(codec.pack_scalars([key_int])[0], b, e, codec.pack_scalars(nonces), gs, dst=DST)
        assert [(p.tobytes(), int(s)) for p, s in zip(out, st)] == want, note
        return st.tolist()

    def check_verify(pk, b, e, proofs, note):
        want = ref.verify(pk, [x.tobytes() for x in b], [x.tobytes() for x in e], [p.tobytes() for p in proofs], DST, gs)
        ok, st = eng.dleq_verify(pk, b, e, proofs, gs, dst=DST)
        assert list(zip(ok.tolist(), st.tolist())) == want, note
        return st.tolist()

    # an undecodable C row: prove and verify, the largest code of the group
    b = good_b.copy()
    b[3] = np.frombuffer(NOT_ON_CURVE, dtype=np.uint8)
    assert check_prove(b, good_e, [11, 12, 13, 14], key, "C") == [0, 16 + 2, 0, 0]
    assert check_verify(pk32, b, good_e, good, "C") == [0, 16 + 2, 0, 0]
    b[2] = np.frombuffer(ref.NEUTRAL32, dtype=np.uint8)
    assert check_prove(b, good_e, [11, 12, 13, 14], key, "C, two codes") == [0, 16 + 3, 0, 0]
    # an undecodable D row: the prover only hashes it, the verifier refuses it
    e = good_e.copy()
    e[4] = np.frombuffer(NOT_ON_CURVE, dtype=np.uint8)
    assert check_prove(good_b, e, [11, 12, 13, 14], key, "D") == [0, 0, 0, 0]
    assert check_verify(pk32, good_b, e, good, "D") == [0, 0, 16 + 2, 0]
    m32, z32, st = eng.dleq_composites(pk32, good_b, e, gs, dst=DST)
    assert st.tolist() == [0, 0, 16 + 2, 0] and not m32[2].any() and not z32[2].any() and m32[[0, 1, 3]].any(axis=1).all()
    # a public key that does not decode marks every group
    assert check_verify(NOT_ON_CURVE, good_b, good_e, good, "pk") == [16 + 2] * 4
    # the key N; the nonces 0 and N
    assert check_prove(good_b, good_e, [11, 12, 13, 14], N, "key N") == [_lib.DH_NEUTRAL] * 4
    assert check_prove(good_b, good_e, [11, 0, N, 14], key, "nonces") == [0, _lib.DLEQ_NONCE_ZERO, _lib.DLEQ_NONCE_ZERO, 0]
    # c >= N
    p = good.copy()
    p[1, :32] = 0xFF
    assert check_verify(pk32, good_b, good_e, p, "c >= N") == [0, _lib.SIG_S_RANGE, 0, 0]


# ---- 5. the _dev forms ----------------------------------------------------------------------------------------------------------------------------
def test_dev_forms_after_reserve_equal_the_host_forms(eng):
    staged(eng)
    groups, gs = 5, 64
    s = shape(groups, gs)
    d_b, d_e, d_r = to_dev(s["b"]), to_dev(s["e"]), to_dev(s["r"])
    eng.dleq_reserve(groups, gs)
    for _ in range(2):                                              # the second call finds everything sized: same results, no error
        proof, ok, st, st2 = dev_full((groups, 64)), dev_full(groups), dev_full(groups), dev_full(groups)
        m32, z32, st3 = dev_full((groups, 32)), dev_full((groups, 32)), dev_full(groups)
        eng.dleq_prove_dev(s["k"], d_b, d_e, d_r, proof, st, groups, gs, dst=DST)
        eng.dleq_verify_dev(s["pk"], d_b, d_e, proof, ok, st2, groups, gs, dst=DST)
        eng.dleq_composites_dev(s["pk"], d_b, d_e, m32, z32, st3, groups, gs, dst=DST)
        eng.sync()
        assert np.array_equal(proof.cpu().numpy(), s["proofs"]) and not st.cpu().numpy().any()
        assert ok.cpu().numpy().tolist() == [1] * groups and not st2.cpu().numpy().any()
        assert np.array_equal(m32.cpu().numpy(), s["m32"]) and np.array_equal(z32.cpu().numpy(), s["z32"]) and not st3.cpu().numpy().any()
    # a smaller shape under the same reservation
    small = shape(3, 5)
    proof, st = dev_full((3, 64)), dev_full(3)
    eng.dleq_prove_dev(small["k"], to_dev(small["b"]), to_dev(small["e"]), to_dev(small["r"]), proof, st, 3, 5, dst=DST)
    eng.sync()
    assert np.array_equal(proof.cpu().numpy(), small["proofs"]) and not st.cpu().numpy().any()


def test_dev_forms_refuse_bad_arguments_and_touch_nothing(eng):
    staged(eng)
    groups, gs = 3, 5
    s = shape(groups, gs)
    d_b, d_e, d_r, d_p = to_dev(s["b"]), to_dev(s["e"]), to_dev(s["r"]), to_dev(s["proofs"])
    proof, ok, st, m32, z32 = dev_full((groups, 64)), dev_full(groups), dev_full(groups), dev_full((groups, 32)), dev_full((groups, 32))
    calls = [lambda: eng.dleq_prove_dev(s["k"], d_b.data_ptr() + 8, d_e, d_r, proof, st, groups, gs, dst=DST),
             lambda: eng.dleq_prove_dev(s["k"], d_b, d_e.data_ptr() + 8, d_r, proof, st, groups, gs, dst=DST),
             lambda: eng.dleq_prove_dev(s["k"], d_b, d_e, d_r.data_ptr() + 8, proof, st, groups, gs, dst=DST),
             lambda: eng.dleq_prove_dev(s["k"], d_b, d_e, d_r, proof.data_ptr() + 8, st, groups, gs, dst=DST),
             lambda: eng.dleq_verify_dev(s["pk"], d_b, d_e, d_p.data_ptr() + 8, ok, st, groups, gs, dst=DST),
             lambda: eng.dleq_verify_dev(s["pk"], d_b.data_ptr() + 8, d_e, d_p, ok, st, groups, gs, dst=DST),
             lambda: eng.dleq_composites_dev(s["pk"], d_b, d_e, m32.data_ptr() + 8, z32, st, groups, gs, dst=DST),
             lambda: eng.dleq_prove_dev(s["k"], d_b, d_e, d_r, proof, st, groups, 0, dst=DST),                # group_size == 0
             lambda: eng.dleq_verify_dev(s["pk"], d_b, d_e, d_p, ok, st, groups, 0, dst=DST),
             lambda: eng.dleq_prove_dev(s["k"], d_b, d_e, d_r, proof, st, groups, gs, dst=b""),               # no DST
             lambda: eng.dleq_prove_dev(s["k"], d_b, d_e, d_r, proof, st, 1 << 40, 1 << 40, dst=DST),         # the product overflows the limit
             lambda: eng.dleq_reserve(groups, 0)]
    for call in calls:
        with pytest.raises(FourQError):
            call()
    eng.dleq_prove_dev(s["k"], d_b, d_e, d_r, proof, st, 0, gs, dst=DST)                                     # groups == 0: fine, nothing touched
    eng.dleq_verify_dev(s["pk"], d_b, d_e, d_p, ok, st, 0, 0, dst=DST)
    eng.dleq_reserve(0, 0)
    eng.sync()
    for t in (proof, ok, st, m32, z32):
        assert (t.cpu().numpy() == 0xAA).all()
    # unaligned ok and status are fine
    ok2, st2 = dev_full(groups + 1), dev_full(groups + 1)
    eng.dleq_verify_dev(s["pk"], d_b, d_e, d_p, ok2.data_ptr() + 1, st2.data_ptr() + 1, groups, gs, dst=DST)
    eng.sync()
    assert ok2.cpu().numpy().tolist() == [0xAA, 1, 1, 1] and st2.cpu().numpy().tolist() == [0xAA, 0, 0, 0]
    assert eng.dleq_prove(s["k"], s["b"][:0], s["e"][:0], s["r"][:0], gs, dst=DST)[0].shape == (0, 64)


def test_prove_and_verify_dev_can_be_captured_into_a_hip_graph(eng):
    """after dleq_reserve and with the comb staged on the capturing stream the two calls only enqueue kernels: one graph proves and checks,
    and a replay over new rows in the captured buffers gives the new rows' proofs"""
    import torch
    dev = torch.device("cuda", 0)
    groups, gs = 3, 5
    s, other = shape(groups, gs), shape(5, 64)
    n = groups * gs
    d_b, d_e, d_r = to_dev(s["b"]), to_dev(s["e"]), to_dev(s["r"])
    proof, pst, ok, vst = dev_full((groups, 64)), dev_full(groups), dev_full(groups), dev_full(groups)
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    try:
        eng.comb_stage(eng.comb_table(G1_WORDS))              # staged on this stream, outside the capture
        eng.dleq_reserve(groups, gs)
        eng.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            eng.dleq_prove_dev(s["k"], d_b, d_e, d_r, proof, pst, groups, gs, dst=DST)
            eng.dleq_verify_dev(s["pk"], d_b, d_e, proof, ok, vst, groups, gs, dst=DST)
            graph.capture_end()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(proof.cpu().numpy(), s["proofs"]) and ok.cpu().numpy().tolist() == [1] * groups
        assert not pst.cpu().numpy().any() and not vst.cpu().numpy().any()
        # rows 64 .. 78 of the pool with the nonces of the first three groups of another shape: not what `shape` holds, so the restatement is asked
        key, pk32, blinded, evaluated = pool()
        b2, e2 = blinded[64:64 + n], evaluated[64:64 + n]
        nonces = codec.unpack_scalars(other["r"][:groups])
        d_b.copy_(to_dev(rows_of(b2, 32))), d_e.copy_(to_dev(rows_of(e2, 32))), d_r.copy_(to_dev(other["r"][:groups]))
        graph.replay()
        torch.cuda.synchronize()
        assert [(p.tobytes(), int(st)) for p, st in zip(proof.cpu().numpy(), pst.cpu().numpy())] == ref.prove(key, b2, e2, [int(v) for v in nonces], DST, gs)
        assert ok.cpu().numpy().tolist() == [1] * groups and not vst.cpu().numpy().any()
    finally:
        eng.set_stream(None)
        _combs.pop(id(eng), None)                             # the next test stages the comb again on the engine's own stream


# ---- 6. between other families on one context, no synchronisation in between -------------------------------------------------------------------
def test_interleaved_with_evaluate_and_signature_checks_without_a_sync(eng):
    staged(eng)
    key, pk32, blinded, evaluated = pool()
    groups, gs = 40, 5
    s = shape(groups, gs)
    n = groups * gs
    # signatures of MORE rows than the proofs have: the signature check's layout then covers what the proofs' stages have left
    n_sig = 300
    rng = np.random.default_rng(7)
    sk, msgs = rng.integers(0, 256, size=(n_sig, 32), dtype=np.uint8), rng.integers(0, 256, size=(n_sig, 48), dtype=np.uint8)
    spk = eng.sig_keygen(sk)
    sigs = eng.sig_sign(sk, spk, msgs)
    sigs[17, 40] ^= 1
    want_sig = np.ones(n_sig, dtype=np.uint8)
    want_sig[17] = 0
    d_b, d_r = to_dev(s["b"]), to_dev(s["r"])
    d_spk, d_msgs, d_sigs = to_dev(spk), to_dev(msgs), to_dev(sigs)
    ev, est = dev_full((n, 32)), dev_full(n)
    proof, pst, ok, vst = dev_full((groups, 64)), dev_full(groups), dev_full(groups), dev_full(groups)
    sok, sst = dev_full(n_sig), dev_full(n_sig)
    eng.dleq_reserve(groups, gs)
    eng.reserve(n_sig)
    eng.sync()
    eng.oprf_evaluate_dev(s["k"], d_b, ev, est, n)
    eng.dleq_prove_dev(s["k"], d_b, ev, d_r, proof, pst, groups, gs, dst=DST)
    eng.sig_verify_dev(d_spk, d_msgs, 48, None, 48, d_sigs, sok, sst, n_sig)
    eng.dleq_verify_dev(pk32, d_b, ev, proof, ok, vst, groups, gs, dst=DST)
    eng.sync()
    assert np.array_equal(ev.cpu().numpy(), s["e"]) and not est.cpu().numpy().any()
    assert np.array_equal(proof.cpu().numpy(), s["proofs"]) and not pst.cpu().numpy().any()
    assert np.array_equal(sok.cpu().numpy(), want_sig) and not sst.cpu().numpy().any()
    assert ok.cpu().numpy().all() and not vst.cpu().numpy().any()


# ---- 7. the bytes module and several devices ---------------------------------------------------------------------------------------------------
def test_bytes_module_round_trip_and_known_answer(eng):
    from fourq_amd import oprf
    key, pk32, blinded, evaluated = pool()
    assert oprf.public_key(key) == pk32 and oprf.public_key(oprf.KAT_KEY).hex() == oprf.KAT_PK
    kat = oprf.prove(oprf.KAT_KEY, [bytes.fromhex(oprf.KAT_BLINDED)], [bytes.fromhex(oprf.KAT_EVALUATED)], oprf.KAT_DST, nonces=[oprf.KAT_NONCE])
    assert [p.hex() for p in kat] == [oprf.KAT_PROOF]
    b, e = blinded[:6], evaluated[:6]
    proofs = oprf.prove(key, b, e, DST, group_size=2)                                # nonces from `secrets`
    assert len(proofs) == 3 and oprf.verify(pk32, b, e, proofs, DST, group_size=2) == [True, True, True]
    one = oprf.prove(key, b, e, DST)                                                 # one group covers everything
    assert len(one) == 1 and oprf.verify(pk32, b, e, one, DST) == [True]
    assert oprf.verify(pk32, b, e[:2] + [e[3], e[2]] + e[4:], proofs, DST, group_size=2) == [True, False, True]
    with pytest.raises(ValueError):
        oprf.prove(key, b, e, DST, group_size=4)
    with pytest.raises(ValueError):
        oprf.verify(pk32, [NOT_ON_CURVE] + b[1:], e, proofs, DST, group_size=2)
    assert oprf.prove(key, [], [], DST) == [] and oprf.verify(pk32, [], [], [], DST) == []


def test_multi_engine_shards_whole_groups(eng):
    from fourq_amd import MultiEngine, device_count
    staged(eng)
    groups, gs = 7, 3
    key, pk32, blinded, evaluated = pool()
    b, e = rows_of(blinded[:groups * gs], 32), rows_of(evaluated[:groups * gs], 32)
    k, r = codec.pack_scalars([key])[0], codec.pack_scalars(list(range(21, 21 + groups)))
    want, wst = eng.dleq_prove(k, b, e, r, gs, dst=DST)
    assert not wst.any() and ref.prove_group(key, blinded[:gs], evaluated[:gs], 21, DST) == (want[0].tobytes(), 0)
    count = device_count()
    with MultiEngine(list(range(count)) if count > 1 else [0, 0]) as multi:
        multi.ct_select = eng.ct_select
        comb = multi.comb_table(G1_WORDS)
        proofs, st = multi.dleq_prove(k, b, e, r, gs, dst=DST, comb=comb)
        assert np.array_equal(proofs, want) and not st.any()
        tampered = proofs.copy()
        tampered[5, 3] ^= 4
        ok, st = multi.dleq_verify(pk32, b, e, tampered, gs, dst=DST, comb=comb)
        assert ok.tolist() == [1, 1, 1, 1, 1, 0, 1] and not st.any()
        assert multi.dleq_public_key(k).tobytes() == pk32
