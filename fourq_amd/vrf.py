"""The verifiable random function on `bytes`, computed on the GPU through the process-wide engine (fourq_vrf_* of include/fourq_amd.h,
where the construction is written out): the holder of a signature key maps a public input to a pseudorandom output and a proof, and
everyone else checks the proof and gets the same output from it.

    pk = schnorrq.keygen(sk)                     the keys are the signature scheme's
    proof = prove(sk, alpha, dst)                key holder; 96 bytes, deterministic (pk is derived unless given)
    beta = verify(pk, alpha, proof, dst)         anyone; 64 bytes, or None when the proof does not hold
    beta == proof_to_hash(proof, dst)            the output of a proof that has been verified

The `_many` forms take lists and make one batched call each.  The suite is this project's own (the structure of RFC 9381's ECVRF with
Elligator 2; no interoperability is claimed); `dst` is the caller's domain separation tag, 1..255 bytes.  A row the library marks (a key
or a Gamma that does not decode, c or s not below N, a Gamma without a component of order N) raises ValueError; a proof that merely does
not hold gives None.  There is no CPU fallback.
"""
import numpy as np

from . import codec
from .schnorrq import _engine, _rows

# one fixed row as the CPU restatement of the construction (tests/vrf_ref.py) gives it: data, for the self-tests
KAT_DST = b"FourQ-VRF-V01-KAT"
KAT_SK = "000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f"
KAT_ALPHA = b"slot 4242 of epoch 17".hex()
KAT_PK = "62624dc8d47b184664fa8b13a54f2e2d58194c577d1c0d59d2fa611a2b2e595a"
KAT_PROOF = ("5b431d0c995915d4fafd03f20bc12356d2830ff105eb28679476d0754e8e71fa"
             "e1b0cc2a70b0e72c9357933869b29ffd175285003235786874b529bb2a9f2000"
             "81bce73db32d55b66f2b7ea70acc8aebfb6b75a07bc9f471b6585595bf1a0700")
KAT_BETA = ("d9bd5294a64189d723f91fa9fe3b1ec8fa9690f669cd8bc7d34d7232425111d7"
            "2c7c64cb2f608fec1f0878460c9cd1c3c104fa06181a0f2797f92719eae8d4f3")


def _checked(status, what):
    bad = np.flatnonzero(status)
    if len(bad):
        raise ValueError("%s: row %d has status %d (include/fourq_amd.h, \"verifiable random function\")" % (what, int(bad[0]), int(status[bad[0]])))


def prove_many(sks, alphas, dst, pks=None):
    """One 96-byte proof per (sk, alpha); `pks`: the matching public keys where the caller has them (derived otherwise)."""
    alphas = [bytes(a) for a in alphas]
    if not alphas:
        return []
    eng, comb = _engine()
    sk = _rows(sks, 32, "a secret key")
    pk = eng.sig_keygen(sk, comb) if pks is None else _rows(pks, 32, "a public key")
    matrix, lens = codec.pack_messages(alphas)
    return [r.tobytes() for r in eng.vrf_prove(sk, pk, matrix, lens, dst=dst, comb=comb)]


def verify_many(pks, alphas, proofs, dst):
    """One entry per (pk, alpha, proof): the 64-byte output, or None where the proof does not hold."""
    alphas = [bytes(a) for a in alphas]
    if not alphas:
        return []
    eng, comb = _engine()
    matrix, lens = codec.pack_messages(alphas)
    beta, ok, status = eng.vrf_verify(_rows(pks, 32, "a public key"), matrix, _rows(proofs, 96, "a proof"), lens, dst=dst, comb=comb)
    _checked(status, "verify")
    return [b.tobytes() if v else None for b, v in zip(beta, ok)]


def proof_to_hash_many(proofs, dst):
    """The 64-byte outputs of proofs that have been verified; c and s are not looked at."""
    proofs = list(proofs)
    if not proofs:
        return []
    eng, _ = _engine()
    beta, status = eng.vrf_proof_to_hash(_rows(proofs, 96, "a proof"), dst=dst)
    _checked(status, "proof_to_hash")
    return [b.tobytes() for b in beta]


def prove(sk, alpha, dst, pk=None):
    return prove_many([sk], [alpha], dst, None if pk is None else [pk])[0]


def verify(pk, alpha, proof, dst):
    return verify_many([pk], [alpha], [proof], dst)[0]


def proof_to_hash(proof, dst):
    return proof_to_hash_many([proof], dst)[0]
