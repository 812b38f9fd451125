"""The argument contract of every grouped call (one output row per group of group_size elements), stated once as a table over the host
forms -- fourq_msm_{affine,bytes}_batch, fourq_bucketsum_{affine,bytes}, fourq_commit_{affine,bytes}, fourq_dleq_{composites,prove,verify}
-- and the three *_reserve calls, in both selection modes:

  * a NULL context or a NULL required pointer is FOURQ_ERR_INVALID, whatever the counts are (also with groups == 0);
  * groups == 0 with valid pointers is FOURQ_OK, whatever group_size is;
  * group_size == 0, or groups x group_size above FOURQ_MAX_BATCH, or a product that wraps (to 0, or to a small number) is FOURQ_ERR_INVALID;
  * none of these calls touches an output byte;
  * a good call at the smallest shapes gives the bytes of its _dev form: (1, 1), (3, 2) and (2, 65), 65 being the smallest group size that
    takes a second fold pass.  The generator set below has 65 bases, so the commitments reach 65 too; the proofs take (1, 1) and (3, 2).

Nothing here is compared with an oracle: the files of the single features do that.  The rows come from the comb, so every point has order N."""
import collections
import ctypes

import numpy as np
import pytest

import curve4q_oracle as o
from bench import seeded_scalars
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu
OK, INVALID = _lib.OK, _lib.ERR_INVALID
FILL = 0xA5
ROWS, BASES = 2 * 65, 65
DST = b"FourQ-grouped-contract-test"
G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
SHAPES = [(1, 1), (3, 2), (2, 65)]                                     # (groups, group_size)
TOO_MANY = [(_lib.MAX_BATCH // 2 + 1, 2), (1 << 63, 2), (((1 << 64) - 1) // 3 + 1, 3)]      # above the limit; wraps to 0; wraps to 2

# One argument behind the context, in the C order.  kind: "in" = an input array of `width` bytes per row (one row per element, or per group
# where per_row is False), "out" = an output array of `width` bytes per group, "ptr" = a required pointer that is no array (the same host
# pointer in the host and the _dev form), "val" = passed as it is.  groups and group_size follow the list, then the call's `tail`.
Arg = collections.namedtuple("Arg", "kind name width per_row", defaults=(0, True))
Call = collections.namedtuple("Call", "name args tail shapes", defaults=((), SHAPES))
SUM_AFFINE = [Arg("in", "k", 32), Arg("in", "P", 64), Arg("out", "out", 64)]
SUM_BYTES = [Arg("in", "k", 32), Arg("in", "enc", 32), Arg("out", "out", 32), Arg("out", "status", 1)]
ROWS_IN = [Arg("ptr", "dst"), Arg("val", "dst_len"), Arg("in", "enc", 32), Arg("in", "evaluated", 32)]
CALLS = [
    Call("fourq_msm_affine_batch", SUM_AFFINE),
    Call("fourq_msm_bytes_batch", SUM_BYTES),
    Call("fourq_bucketsum_affine", SUM_AFFINE, (4,)),                  # window 4: the bucket route (the ladder route in constant-time mode)
    Call("fourq_bucketsum_bytes", SUM_BYTES, (4,)),
    Call("fourq_commit_affine", [Arg("in", "k", 32), Arg("out", "out", 64)], (0,)),
    Call("fourq_commit_bytes", [Arg("in", "k", 32), Arg("out", "out", 32)], (0,)),
    Call("fourq_dleq_composites", ROWS_IN[:2] + [Arg("ptr", "pk")] + ROWS_IN[2:] + [Arg("out", "m32", 32), Arg("out", "z32", 32), Arg("out", "status", 1)], (), SHAPES[:2]),
    Call("fourq_dleq_prove", [Arg("ptr", "key"), Arg("val", "comb")] + ROWS_IN + [Arg("in", "nonces", 32, False), Arg("out", "proofs", 64), Arg("out", "status", 1)], (), SHAPES[:2]),
    Call("fourq_dleq_verify", [Arg("ptr", "pk"), Arg("val", "comb")] + ROWS_IN + [Arg("in", "proofs", 64, False), Arg("out", "ok", 1), Arg("out", "status", 1)], (), SHAPES[:2]),
]
RESERVES = [("fourq_bucketsum_reserve", (4,)), ("fourq_bucketsum_reserve", (0,)), ("fourq_commit_reserve", ()), ("fourq_dleq_reserve", ())]
_cache = {}


def data(eng):
    """ROWS points [t_i]G with their encodings and evaluations under one key, scalars, nonces, and the first BASES points as the context's
    generator set; the generator's comb staged (the proofs pass comb = NULL).  Once per engine, never changed."""
    if id(eng) not in _cache:
        comb = eng.comb_table(G1_WORDS)
        eng.comb_stage(comb)
        P, st = eng.comb_mul(seeded_scalars(8101, ROWS), comb)
        assert not st.any()
        key = seeded_scalars(8102, 1)[0]
        enc = eng.encode(P)
        evaluated, st = eng.oprf_evaluate(key, enc)
        assert not st.any()
        eng.commit_bases(P[:BASES])
        dst = ctypes.create_string_buffer(DST, len(DST))
        _cache[id(eng)] = {"k": seeded_scalars(8103, ROWS), "P": P, "enc": enc, "evaluated": evaluated, "key": key.copy(), "pk": eng.dleq_public_key(key),
                           "nonces": seeded_scalars(8104, 3), "proofs": np.zeros((3, 64), dtype=np.uint8),      # proofs: rows for the calls that are refused
                           "dst": dst, "dst_len": len(DST), "comb": None}
    return _cache[id(eng)]


def address(x):
    if x is None or isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr() if hasattr(x, "data_ptr") else ctypes.addressof(x)


def host_args(d, call, groups, group_size):
    """the call's arguments over host arrays: ([argument or array], {name: output array prefilled with FILL})"""
    n, outs, args = groups * group_size, {}, []
    for a in call.args:
        if a.kind == "in":
            args.append(np.ascontiguousarray(d[a.name][:n if a.per_row else groups]))
        elif a.kind == "out":
            outs[a.name] = np.full((groups, a.width), FILL, dtype=np.uint8)
            args.append(outs[a.name])
        else:
            args.append(d[a.name])
    return args, outs


def invoke(fn, ctx, args, groups, group_size, tail):
    return fn(ctx, *[address(x) for x in args], groups, group_size, *tail)


@pytest.mark.parametrize("call", CALLS, ids=[c.name for c in CALLS])
def test_bad_arguments_are_refused_and_touch_nothing(eng, call):
    d = data(eng)
    fn, ctx = getattr(eng._lib, call.name), eng._ctx
    args, outs = host_args(d, call, 3, 2)
    pointers = [i for i, a in enumerate(call.args) if a.kind != "val"]
    assert len(pointers) >= 2
    for groups, group_size in [(3, 2), (0, 2), (0, 0)]:                 # the pointers are looked at first: groups == 0 excuses none of them
        assert invoke(fn, None, args, groups, group_size, call.tail) == INVALID, (groups, group_size)
        for i in pointers:
            assert invoke(fn, ctx, args[:i] + [None] + args[i + 1:], groups, group_size, call.tail) == INVALID, (call.args[i].name, groups, group_size)
    assert invoke(fn, ctx, args, 3, 0, call.tail) == INVALID and invoke(fn, ctx, args, 1, 0, call.tail) == INVALID
    for groups, group_size in TOO_MANY:
        assert invoke(fn, ctx, args, groups, group_size, call.tail) == INVALID, (groups, group_size)
    for group_size in (0, 4):
        assert invoke(fn, ctx, args, 0, group_size, call.tail) == OK, group_size
    eng.sync()
    for name, out in outs.items():
        assert (out == FILL).all(), name


@pytest.mark.parametrize("name,tail", RESERVES, ids=["%s-%s" % (n, "-".join(map(str, t)) or "x") for n, t in RESERVES])
def test_reserve_calls_keep_the_same_rules(eng, name, tail):
    fn, ctx = getattr(eng._lib, name), eng._ctx
    for groups, group_size in [(3, 2), (0, 2), (0, 0)]:
        assert fn(None, groups, group_size, *tail) == INVALID, (groups, group_size)
    assert fn(ctx, 3, 0, *tail) == INVALID and fn(ctx, 1, 0, *tail) == INVALID
    for groups, group_size in TOO_MANY:
        assert fn(ctx, groups, group_size, *tail) == INVALID, (groups, group_size)
    for group_size in (0, 4):
        assert fn(ctx, 0, group_size, *tail) == OK, group_size
    assert fn(ctx, 3, 2, *tail) == OK


@pytest.mark.parametrize("call", CALLS, ids=[c.name for c in CALLS])
def test_host_form_equals_dev_form(eng, call):
    import torch
    d = data(eng)
    host, dev, ctx = getattr(eng._lib, call.name), getattr(eng._lib, call.name + "_dev"), eng._ctx
    for groups, group_size in call.shapes:
        if call.name == "fourq_dleq_verify":                            # the proofs of this shape: the host form's, which the prover's _dev form equals
            prove = CALLS[-2]
            args, outs = host_args(d, prove, groups, group_size)
            assert invoke(getattr(eng._lib, prove.name), ctx, args, groups, group_size, prove.tail) == OK and not outs["status"].any()
            d = dict(d, proofs=outs["proofs"])
        args, outs = host_args(d, call, groups, group_size)
        assert invoke(host, ctx, args, groups, group_size, call.tail) == OK, (groups, group_size)
        dev_args, dev_outs = [], {}
        for a, x in zip(call.args, args):
            if a.kind == "in":
                x = torch.from_numpy(x.view(np.uint8).reshape(-1)).to(torch.device("cuda", 0))
            elif a.kind == "out":
                x = dev_outs[a.name] = torch.full((groups, a.width), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
            dev_args.append(x)
        assert invoke(dev, ctx, dev_args, groups, group_size, call.tail) == OK, (groups, group_size)
        eng.sync()
        for name, out in outs.items():
            assert np.array_equal(out, dev_outs[name].cpu().numpy()), (name, groups, group_size)
        assert not (outs[call.args[-1].name] == FILL).all()                                       # the last output, at least, was written
        if "status" in outs:
            assert not outs["status"].any(), (groups, group_size)
        if "ok" in outs:
            assert (outs["ok"] == 1).all(), (groups, group_size)
