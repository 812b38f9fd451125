"""The signature scheme's restatement (tests/sig_ref.py) on the CPU: against the rows the real reference's point functions produced
(tests/golden/schnorrq.json), round trips, every tamper class the GPU tests use, and the C-oracle-accelerated batch form."""
import random

import numpy as np

import curve4q_oracle as o
import sig_ref as ref

LENGTHS = [0, 1, 15, 16, 17, 47, 48, 79, 80, 111, 112, 127, 128, 129, 1000]


def rows(golden):
    return [{k: (v if k.startswith("_") else bytes.fromhex(v)) for k, v in r.items()} for r in golden("schnorrq.json", raw=True)["rows"]]


def test_restatement_reproduces_the_golden_rows(golden):
    cases = rows(golden)
    assert len(cases) >= 40
    assert {len(c["msg"]) for c in cases} >= set(LENGTHS)
    assert sum(1 for c in cases if c["_a_ge_N"]) >= 30 and sum(1 for c in cases if not c["_a_ge_N"]) >= 2
    for c in cases:
        assert (ref.LE(ref.H(c["sk"])[:32]) >= o.N) == c["_a_ge_N"]
        assert ref.keygen(c["sk"]) == c["pk"], c["_label"]
        assert ref.sign(c["sk"], c["pk"], c["msg"]) == c["sig"], c["_label"]
        assert ref.verify(c["pk"], c["msg"], c["sig"]) == (1, 0), c["_label"]


def test_unreduced_scalar_is_the_reduced_one_on_the_curve():
    rng = random.Random(1)
    for _ in range(3):
        k = rng.getrandbits(256) | (1 << 255)
        assert ref.mul_g_encoded(k) == ref.mul_g_encoded(k % o.N)


def tampered(pk, msg, sig, how, refused):
    """One row spoiled in the way `how` names: (pk, msg, sig)."""
    pk, sig, m = bytearray(pk), bytearray(sig), bytearray(msg)
    if how == "msg bit":
        m[len(m) // 2] ^= 4
    elif how == "R bit":
        sig[7] ^= 1
    elif how == "s bit":
        sig[32 + 3] ^= 8
    elif how == "pk bit":
        pk[20] ^= 2
    elif how == "s + N":
        sig[32:] = (ref.LE(sig[32:]) + o.N).to_bytes(32, "little")
    elif how == "pk reserved bit":
        pk[15] |= 0x80
    elif how == "pk off curve":
        pk[:] = refused
    elif how == "length one short":
        m = m[:-1]
    else:
        raise ValueError(how)
    return bytes(pk), bytes(m), bytes(sig)


TAMPERS = ["msg bit", "R bit", "s bit", "pk bit", "s + N", "pk reserved bit", "pk off curve", "length one short"]


def off_curve_key(golden):
    bad = [bytes.fromhex(r[0]) for r in golden("wire.json", raw=True)["strings"] if r[1] == "Exception" and "not on curve" in r[2]]
    assert bad
    return bad[0]


def test_every_tamper_class_is_rejected_by_the_restatement(golden):
    cases = [c for c in rows(golden) if len(c["msg"]) >= 2][:8]
    refused = off_curve_key(golden)
    for c, how in zip(cases, TAMPERS):
        ok, st = ref.verify(*tampered(c["pk"], c["msg"], c["sig"], how, refused))
        assert ok == 0, how
        if how == "s + N":
            assert st == ref.SIG_S_RANGE and ref.LE(c["sig"][32:]) + o.N < 1 << 256
        elif how == "pk reserved bit":
            assert st == ref.BYTES_DECODE_BASE + ref.DECODE_RESERVED_BIT
        elif how == "pk off curve":
            assert st == ref.BYTES_DECODE_BASE + ref.DECODE_NOT_ON_CURVE
        elif how == "pk bit":
            assert st in (0, ref.BYTES_DECODE_BASE + ref.DECODE_NOT_ON_CURVE, ref.BYTES_DECODE_BASE + ref.DECODE_RESERVED_BIT)
        else:
            assert st == 0, how
    # a key that does not decode takes precedence over the range of s
    c = cases[0]
    pk, m, sig = tampered(c["pk"], c["msg"], c["sig"], "s + N", refused)
    assert ref.verify(tampered(pk, m, sig, "pk reserved bit", refused)[0], m, sig) == (0, ref.BYTES_DECODE_BASE + ref.DECODE_RESERVED_BIT)


def test_batch_form_is_the_restatement():
    rng = random.Random(20261017)
    sks = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(64)]
    msgs = [bytes(rng.getrandbits(8) for _ in range(rng.choice(LENGTHS + [rng.randrange(300)]))) for _ in range(64)]
    pks = ref.batch_keygen(sks)
    sigs = ref.batch_sign(sks, [p.tobytes() for p in pks], msgs)
    assert pks.dtype == np.uint8 and pks.shape == (64, 32) and sigs.shape == (64, 64)
    for i in range(64):
        assert pks[i].tobytes() == ref.keygen(sks[i])
        assert sigs[i].tobytes() == ref.sign(sks[i], pks[i].tobytes(), msgs[i])
    for i in range(0, 64, 9):
        assert ref.verify(pks[i].tobytes(), msgs[i], sigs[i].tobytes()) == (1, 0)
