"""The fixed-generator commitments (fourq_commit_*, fourq_amd/csrc/commit.hip.h) restated on the Python oracle: out[g] is
R1toAffine of the sum over j of MUL_endo(k_gj, AffineToR1(B_j)), the sum taken with the complete addition -- what fourq_msm_* computes
over the bases tiled `groups` times, and what the combs must reproduce bit for bit for bases of order N.  No GPU, nothing from the
library under test."""
import curve4q_oracle as o

NEUTRAL_AFFINE = ((0, 0), (1, 0))


def commit(scalars, bases, group_size):
    """canonical affine commitments of the rows of `scalars` (ints, group after group) over the first group_size `bases` (affine tuples)"""
    assert 1 <= group_size <= len(bases) and len(scalars) % group_size == 0
    lifted = [o.AffineToR1(*B) for B in bases[:group_size]]
    out = []
    for g in range(len(scalars) // group_size):
        acc = None
        for j, B in enumerate(lifted):
            T = o.MUL_endo(scalars[g * group_size + j], B)
            acc = T if acc is None else o.ADD(acc, o.R1toR2(T))
        out.append(o.R1toAffine(acc))
    return out


def commit_bytes(scalars, bases, group_size):
    return [bytes(bytearray(o.encode(*P))) for P in commit(scalars, bases, group_size)]


def multiple_of_g(s):
    """[s mod N]G, canonical affine: the group-law expectation for bases [t_j]G is multiple_of_g(sum_j k_j t_j)"""
    return o.R1toAffine(o.MUL_endo(s % o.N, o.AffineToR1(o.Gx, o.Gy)))


def closing_scalar(ks, ts):
    """the k for the base after ts[:len(ks)] that makes sum k_j t_j = 0 (mod N): the group commits to the neutral"""
    partial = sum(k * t for k, t in zip(ks, ts))
    return -partial * pow(ts[len(ks)], -1, o.N) % o.N
