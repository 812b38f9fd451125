"""Threshold sharing on `int` and `bytes`, computed on the GPU through the process-wide engine (fourq_shamir_* of include/fourq_amd.h,
"threshold sharing"): a scalar modulo the group order N is split t-of-n with Shamir's scheme, the dealer's Feldman commitments let every
party check its share, and any t parties combine -- their shares, or points each has multiplied by its share.

    shares, commits = split(secret, t, ids)              dealer: {id: share}, t commitments of 32 bytes
    verify_share(commits, id, share)                     party `id`: True iff the share lies on the committed polynomial
    combine({id: share, ...}) == secret % N              any t parties
    combine_points({id: encode([share]P), ...})          the same "in the exponent": encode([secret]P) from t points

A threshold OPRF is `oprf.evaluate` on each server with its share as the key, then `combine_points` over the replies, then
`oprf.finalize`: byte for byte what the undivided key gives.

Ids are integers in [1, 2^32).  The library has no random numbers: `split` draws the t - 1 upper coefficients with
`secrets.randbelow`, here and nowhere deeper; `shares_of` takes them from the caller.  A set the library marks (an id 0, a repeated id,
a point that does not decode) raises ValueError.  There is no CPU fallback.
"""
import secrets

import numpy as np

from . import _lib, codec
from .constants import N
from .schnorrq import _engine, _rows


def _checked(status, what):
    bad = np.flatnonzero(np.atleast_1d(status))
    if len(bad):
        raise ValueError("%s: entry %d has status %d (include/fourq_amd.h, \"threshold sharing\")" % (what, int(bad[0]), int(np.atleast_1d(status)[bad[0]])))


def _id_list(ids):
    ids = [int(i) for i in ids]
    if any(not 0 < i < 1 << 32 for i in ids):
        raise ValueError("an id is an integer in [1, 2^32)")
    return ids


def shares_of(coeffs, ids):
    """{id: f(id) mod N} for the polynomial with the integer coefficients `coeffs` (coeffs[0] is the secret)."""
    ids = _id_list(ids)
    eng, _ = _engine()
    a = codec.pack_scalars([int(c) % (1 << 256) for c in coeffs]).reshape(1, len(coeffs), 4)
    shares, status = eng.shamir_shares(a, ids)
    _checked(status, "shares")
    return dict(zip(ids, codec.unpack_scalars(shares.reshape(len(ids), 4))))


def commitments(coeffs):
    """The Feldman commitments encode([a_j]G) of one polynomial: t strings of 32 bytes.  A coefficient that is 0 mod N has no commitment
    a verifier accepts (the neutral point's encoding does not decode): draw them from [1, N)."""
    eng, comb = _engine()
    a = codec.pack_scalars([int(c) % (1 << 256) for c in coeffs]).reshape(1, len(coeffs), 4)
    return [r.tobytes() for r in eng.shamir_commitments(a, comb)[0]]


def split(secret, t, ids):
    """({id: share}, commitments) of a fresh polynomial of degree t - 1 with f(0) = secret: any t of the shares give the secret back."""
    if not 1 <= int(t) <= _lib.SHAMIR_MAX_T:
        raise ValueError("the threshold is in [1, %d]" % _lib.SHAMIR_MAX_T)
    coeffs = [int(secret)] + [1 + secrets.randbelow(N - 1) for _ in range(int(t) - 1)]
    return shares_of(coeffs, ids), commitments(coeffs)


def public_share(commits, party_id):
    """encode([f(id)]G) from the commitments alone: what `verify_share` compares with, and [1 / 392] of party `id`'s DLEQ public key."""
    (party_id,) = _id_list([party_id])
    eng, _ = _engine()
    out, status = eng.shamir_public_shares(_rows(commits, 32, "a commitment").reshape(1, len(commits), 32), [party_id])
    _checked(status, "public_share")
    return out[0].tobytes()


def verify_share(commits, party_id, share):
    """True iff `share` is the committed polynomial's value at `party_id`."""
    (party_id,) = _id_list([party_id])
    eng, comb = _engine()
    s = codec.pack_scalars([int(share)])
    ok, status = eng.shamir_verify(_rows(commits, 32, "a commitment").reshape(1, len(commits), 32), [party_id], s, comb)
    if status[0] == _lib.SIG_S_RANGE:
        return False
    _checked(status, "verify_share")
    return bool(ok[0])


def lagrange(ids):
    """{id: lambda_id}, the coefficients at 0 of the set `ids`."""
    ids = _id_list(ids)
    eng, _ = _engine()
    lam, status = eng.shamir_lagrange(np.array([ids], dtype=np.uint32))
    _checked(status, "lagrange")
    return dict(zip(ids, codec.unpack_scalars(lam[0])))


def combine(shares):
    """f(0) mod N from {id: share} of t parties."""
    ids = _id_list(shares)
    eng, _ = _engine()
    out, status = eng.shamir_combine(ids, codec.pack_scalars([int(shares[i]) for i in ids]).reshape(len(ids), 1, 4))
    _checked(status, "combine")
    return codec.unpack_scalars(out)[0]


def combine_points_many(points):
    """{id: [32-byte points]} of t parties, every list of one length -> the list of encode(sum_i [lambda_i]P_i) per row."""
    ids = _id_list(points)
    eng, _ = _engine()
    blocks = np.stack([_rows(points[i], 32, "a point") for i in ids])
    out, status = eng.shamir_combine_points(ids, blocks)
    _checked(status, "combine_points")
    return [r.tobytes() for r in out]


def combine_points(points):
    """{id: 32-byte point} of t parties -> encode(sum_i [lambda_i]P_i)."""
    return combine_points_many({i: [p] for i, p in points.items()})[0]
