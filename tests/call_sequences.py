"""Helper of tests/test_gpu_call_sequences.py: a table of step kinds -- one per family of `_dev` entry points, plus the changes of a
context's state -- each of which builds a Plan: the host arrays of one call, the expected bytes of every output, and the call itself.
A run uploads every plan's inputs, allocates every output pre-filled with 0xA5, enqueues the calls with nothing in between, synchronises
the engine ONCE and compares.

Expected values never come from the library: the C oracle (oracle/oracle_c.py) with the modular arithmetic in Python integers -- group-law
identities such as [k]B + [l][t]G = [(k c + l t) mod N]G for B = [c]G -- hashlib, pow, and the restatements tests/sig_ref.py, tests/h2c_ref.py
and tests/oprf_ref.py through the cached seeded batches of their GPU test modules.  Tables and combs are the oracle's too (data only).
Everything is computed once per process and shared by all engines and both selection modes."""
import functools
import hashlib
import random

import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_flags, seeded_scalars
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu

N = o.N
FILL = 0xA5
RESTATED = 257                       # rows of the calls whose expectation is a Python restatement
T2, T3 = 0x5EED0002F00D << 64 | 0x1234567, 0x5EED0003BEEF << 96 | 0x7654321     # P2 = [T2]G, P3 = [T3]G
G1_WORDS = codec.pack_point(o.AffineToR1(o.Gx, o.Gy))
ENTRY = "fourq_%s_batch_dev"


def comb_scalars():
    """the multiple of the base each of the comb's 1 024 + 80 entries holds (include/fourq_amd.h, tests/test_gpu_comb.py)"""
    ms = []
    for t in range(_lib.COMB_POINTS):
        (W, _, E, D), s = ((9, 4, 7, 28), t) if t < 1024 else ((5, 5, 10, 50), t - 1024)
        j, u = s >> (W - 1), s & ((1 << (W - 1)) - 1)
        ms.append((1 << (E * j)) * (1 + sum(((u >> r) & 1) << (D * (r + 1)) for r in range(W - 1))) % N)
    return codec.pack_scalars(ms)


class Base:
    """One base point [c]G: its R1 words, affine words, both tables and (on demand) its comb, all from the C oracle."""

    def __init__(self, c, table_g):
        self.c = c
        self.r1 = G1_WORDS.copy() if c == 1 else oc.mul(oc.ENDO, codec.pack_scalars([c]), None, table_g)[0].copy()
        self.aff = oc.r1_to_affine(self.r1.reshape(1, 20))[0]
        self.te, self.tw = oc.table(oc.ENDO, self.r1), oc.table(oc.WINDOWED, self.r1)

    @functools.cached_property
    def comb(self):
        pts = codec.unpack_points(oc.r1_to_affine(oc.mul(oc.ENDO, comb_scalars(), None, self.te)))
        rows = [(o.f2_add(x, y), o.f2_sub(y, x), o.f2_mul(o.TWO_D, o.f2_mul(x, y))) for x, y in pts]
        return np.ascontiguousarray(codec.pack_points(rows, 3).ravel())


class Data:
    """`rows` seeded scalars k, l and points P_i = [t_i]G with the oracle's answers of the variable-base calls over all of them; the
    steps take slices."""

    def __init__(self, rows):
        self.rows = rows
        self.bases = {}
        g = self.bases["G"] = Base(1, oc.table(oc.ENDO, G1_WORDS))
        for name, c in (("P2", T2), ("P3", T3), ("G392", 392), ("P2x392", 392 * T2 % N)):
            self.bases[name] = Base(c, g.te)
        self.k, self.l, self.t = seeded_scalars(9101, rows), seeded_scalars(9102, rows), seeded_scalars(9103, rows)
        self.ki, self.li, self.ti = (codec.unpack_scalars(x) for x in (self.k, self.l, self.t))
        self.p_r1 = oc.mul(oc.ENDO, self.t, None, g.te)
        self.p_aff = oc.r1_to_affine(self.p_r1)
        self.p_enc = np.ascontiguousarray(oc.encode(self.p_aff))
        self.var_r1 = oc.mul(oc.ENDO, self.k, self.p_r1)
        self.var_aff = oc.r1_to_affine(self.var_r1)
        self.var_enc = np.ascontiguousarray(oc.encode(self.var_aff))
        self.dh_var, st = oc.dh(oc.ENDO, self.k, self.p_aff)
        assert not st.any()
        self.flags = seeded_flags(9104, rows)

    def multiples_of_g(self, ints):
        return oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars([v % N for v in ints]), None, self.bases["G"].te))


_data = {}


def data(rows):
    """The pool, at least `rows` long; a longer one replaces a shorter one (the scalars are a prefix of each other's)."""
    have = max(_data, default=0)
    if have < rows:
        _data.clear()
        _data[rows] = Data(rows)
        have = rows
    return _data[have]


@functools.lru_cache(maxsize=None)
def refused_rows(rows):
    """`rows` 32-byte strings the reference's decode refuses, codes 1, 2, 3 in turn, and 16 + code per row"""
    from test_gpu_msm import refused
    bad = refused()
    enc = np.stack([bad[1 + i % 3][(i // 3) % len(bad[1 + i % 3])] for i in range(rows)]).astype(np.uint8)
    return enc, np.array([_lib.BYTES_DECODE_BASE + 1 + i % 3 for i in range(rows)], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def sig_batch():
    from test_gpu_sig import seeded_batch
    sk, msgs, pks, sigs = seeded_batch(RESTATED, 6100)
    matrix, lens = codec.pack_messages(msgs)
    return {"sk": sk, "msgs": msgs, "pk": pks, "sig": sigs, "m": matrix, "lens": lens}


@functools.lru_cache(maxsize=None)
def sig_verdict(row, spoil):
    """the restatement's (ok, status) of row `row` with R spoiled, or with a key that does not decode"""
    import sig_ref
    c = sig_batch()
    pk, sig = c["pk"][row].tobytes(), bytearray(c["sig"][row].tobytes())
    if spoil == "R":
        sig[5] ^= 1
    else:
        pk = refused_rows(RESTATED)[0][row].tobytes()
    return sig_ref.verify(pk, c["msgs"][row], bytes(sig))


@functools.lru_cache(maxsize=None)
def h2c_batch():
    import h2c_ref
    import test_gpu_h2c as h
    m, lens = h.mixed_batch()
    m, lens, dst = np.ascontiguousarray(m[:RESTATED]), lens[:RESTATED].copy(), h.DSTS[43]
    out = {"m": m, "lens": lens, "dst": dst}
    for mode in ("ro", "nu"):
        out["u_" + mode] = h.want_u_words(m, lens, dst, mode)
        out["aff_" + mode] = h.want_affine_words(m, lens, dst, mode)
        out["enc_" + mode] = np.ascontiguousarray(h.want_bytes(m, lens, dst, mode))
    out["map"] = h.words([h2c_ref.affine_words(h.want_map(h.want_u(m[i, :lens[i]].tobytes(), dst, "nu")[0])) for i in range(RESTATED)])
    return out


@functools.lru_cache(maxsize=None)
def oprf_batch():
    import test_gpu_oprf as t
    c = dict(t.batch())
    c["dst"] = t.DST
    return c


@functools.lru_cache(maxsize=None)
def oprf_rejected(rows):
    """finalize and evaluate on elements that do not decode, by the restatement (it stops at the decode)"""
    import oprf_ref
    c = oprf_batch()
    bad, _ = refused_rows(RESTATED)
    fin = [oprf_ref.finalize(c["m160"][i, :c["lens"][i]].tobytes(), c["dst"], c["blinds"][i], bad[i].tobytes()) for i in range(rows)]
    ev = [oprf_ref.evaluate(c["key"], bad[i].tobytes()) for i in range(rows)]
    rows_of = lambda items, w: np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), w).copy()
    return (rows_of([f[0] for f in fin], 64), np.array([f[1] for f in fin], dtype=np.uint8),
            rows_of([e[0] for e in ev], 32), np.array([e[1] for e in ev], dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def sha_batch():
    rows, stride = 4099, 160
    m = np.random.default_rng(9105).integers(0, 256, size=(rows, stride), dtype=np.uint8)
    lens = np.random.default_rng(9106).integers(0, stride + 1, size=rows, dtype=np.uint32)
    lens[:6] = (0, 111, 112, 127, 128, 160)
    want = np.frombuffer(b"".join(hashlib.sha512(m[i, :lens[i]].tobytes()).digest() for i in range(rows)), dtype=np.uint8).reshape(rows, 64).copy()
    return m, lens, want


@functools.lru_cache(maxsize=None)
def fp2_mul_rows(rows):
    """`rows` inputs of the FP2_MUL primitive (1 000 distinct, repeated) and the oracle's products"""
    rng = random.Random(9107)
    elems = [[(rng.getrandbits(127), rng.getrandbits(127)), (rng.getrandbits(127), rng.getrandbits(127))] for _ in range(min(rows, 1000))]
    x = codec.pack_points(elems, 2)
    want = codec.pack_points([(o.f2_mul(a, b),) for a, b in elems], 1)
    reps = -(-rows // len(elems))
    return np.tile(x, (reps, 1))[:rows].copy(), np.tile(want, (reps, 1))[:rows].copy()


# ---- plans and runs ---------------------------------------------------------------------------------------------------------------------
class State:
    """What the builders need to know of the context's history to say what a call must return: which comb `comb == NULL` means."""

    def __init__(self):
        self.comb = None
        self.side = False


class Plan:
    def __init__(self, kind, n, ins, wants, call, host_wants=(), note=""):
        self.kind, self.n, self.ins, self.wants, self.call, self.host_wants, self.note = kind, n, ins, wants, call, host_wants, note


class Runtime:
    """what the calls of a run share: the external stream the context is switched to, and the statistics of its host-array calls"""

    def __init__(self):
        import torch
        self.side = torch.cuda.Stream(device=torch.device("cuda", 0))
        self.host_stats = []


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", 0))


def differing_rows(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return np.arange(len(want))
    return np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))


class Live:
    def __init__(self, plan):
        import torch
        self.plan = plan
        self.ins = [to_dev(a) for a in plan.ins]
        self.outs = [torch.full((max(16, want.nbytes),), FILL, dtype=torch.uint8, device=torch.device("cuda", 0)) for _, want in plan.wants]
        self.host = None

    def failures(self, index):
        p, out = self.plan, []
        got = [t.cpu().numpy()[:want.nbytes].view(want.dtype).reshape(want.shape) for t, (_, want) in zip(self.outs, p.wants)]
        host = list(self.host or ())
        if len(host) != len(p.host_wants):
            out.append("step %d %s n=%d %s: %d host results for %d expectations" % (index, p.kind, p.n, p.note, len(host), len(p.host_wants)))
        for (label, want), g in list(zip(p.wants, got)) + list(zip(p.host_wants, host)):
            bad = differing_rows(g, want)
            if bad.size:
                out.append("step %d %s n=%d %s: %s differs in %d rows, first %s" % (index, p.kind, p.n, p.note, label, bad.size, bad[:4].tolist()))
        return out


def run(eng, plans, rt=None, sync_each=False):
    """Upload and allocate everything, then enqueue every step with nothing in between, ONE eng.sync(), then compare every step's bytes."""
    import torch
    rt = rt or Runtime()
    live = [Live(p) for p in plans]
    torch.cuda.synchronize()                         # the uploads and fills ran on torch's stream: done before the first enqueue
    for s in live:
        s.host = s.plan.call(eng, rt, s.ins, s.outs)
        if sync_each:
            eng.sync()
    eng.sync()
    failed = [f for i, s in enumerate(live) for f in s.failures(i)]
    assert not failed, "\n".join(failed[:12])
    return live


# ---- the step kinds ---------------------------------------------------------------------------------------------------------------------
KINDS = {}


class Kind:
    def __init__(self, name, entries, cap, build):
        self.name, self.entries, self.cap, self.build = name, entries, cap, build


def kind(name, entries=(), cap=None):
    def deco(fn):
        KINDS[name] = Kind(name, tuple(ENTRY % e for e in entries), cap, fn)
        return fn
    return deco


def build(name, n, st, rng=None, **kw):
    k = KINDS[name]
    assert k.cap is None or n <= k.cap, (name, n)
    rng = rng or random.Random(0)
    d = data(4099 if name in STATE_KINDS else max(n, 4099))      # the host calls of STATE_KINDS repeat the pool past its end
    return k.build(d, n, st, rng, **kw)


def opt(kw, key, rng, choices):
    return kw[key] if key in kw else rng.choice(choices)


def offset(kw, rng, n, rows):
    """where a step's rows start in the pool: within its first 4 099 rows (however long the pool is, so that a seed means one sequence);
    a larger batch starts at row 0"""
    return kw["off"] if "off" in kw else rng.randrange(max(n, min(rows, 4099)) - n + 1)


def producer(kw, st, rng):
    """whether the step's scalars are finished by an add_ on the external stream directly in front of the call: as asked, or -- in a seeded
    sequence -- every other time while the context is on that stream"""
    return kw["producer"] if "producer" in kw else st.side and rng.random() < 0.5


def zeros(n):
    return np.zeros(n, dtype=np.uint8)


def comb_of(d, st, kw, rng, choices=("G", "P2")):
    """(the comb argument: words or None, the base it stands for); a comb given by value becomes the staged one"""
    name = opt(kw, "comb", rng, (None,) + tuple(choices)) if st.comb in choices else opt(kw, "comb", rng, choices)
    if name is None:
        assert st.comb is not None
        return None, d.bases[st.comb], "comb=None (%s)" % st.comb
    st.comb = name
    return d.bases[name].comb, d.bases[name], "comb=%s" % name


@kind("mul_r1", ("mul_endo", "mul_windowed"))
def _(d, n, st, rng, **kw):
    algo, off = opt(kw, "algo", rng, ("endo", "windowed")), offset(kw, rng, n, d.rows)
    k, p = d.k[off:off + n], d.p_r1[off:off + n]
    want = d.var_r1[off:off + n] if algo == "endo" else oc.mul(oc.WINDOWED, k, p)
    if producer(kw, st, rng):                        # the scalars reach their values through an add on the external stream, right before the call
        less = k.copy()
        less[:, 0] -= np.uint64(1)
        one = np.zeros_like(k)
        one[:, 0] = 1

        def call(eng, rt, i, out):
            import torch
            with torch.cuda.stream(rt.side):
                i[0].add_(i[2])
            (eng.mul_endo_dev if algo == "endo" else eng.mul_windowed_dev)(i[0], i[1], out[0], n)
        return Plan("mul_r1", n, [less, p, one], [("out_r1", want)], call, note=algo + " after a producer")
    return Plan("mul_r1", n, [k, p], [("out_r1", want)], lambda eng, rt, i, out: (eng.mul_endo_dev if algo == "endo" else eng.mul_windowed_dev)(i[0], i[1], out[0], n), note=algo)


@kind("mul_affine", ("mul_endo_affine", "mul_windowed_affine"))
def _(d, n, st, rng, **kw):
    algo, off = opt(kw, "algo", rng, ("endo", "windowed") if n <= 4099 else ("endo",)), offset(kw, rng, n, d.rows)
    k, p = d.k[off:off + n], d.p_aff[off:off + n]
    want = d.var_aff[off:off + n] if algo == "endo" else oc.r1_to_affine(oc.mul(oc.WINDOWED, k, d.p_r1[off:off + n]))
    return Plan("mul_affine", n, [k, p], [("out_affine", want)], lambda eng, rt, i, out: eng.mul_affine_dev(i[0], i[1], out[0], n, kind=algo), note=algo)


@kind("mul_bytes", ("mul_endo_bytes", "mul_windowed_bytes"))
def _(d, n, st, rng, **kw):
    algo, off = opt(kw, "algo", rng, ("endo", "windowed")), offset(kw, rng, n, d.rows)
    k = d.k[off:off + n]
    if kw.get("bad"):                                # every point undecodable: the decode codes 1, 2, 3 stay behind in the work buffer
        enc, st_want = refused_rows(RESTATED)
        p, want, st_want = enc[:n], np.zeros((n, 32), dtype=np.uint8), st_want[:n]
    else:
        p, st_want = d.p_enc[off:off + n], zeros(n)
        want = d.var_enc[off:off + n] if algo == "endo" else np.ascontiguousarray(oc.encode(oc.r1_to_affine(oc.mul(oc.WINDOWED, k, d.p_r1[off:off + n]))))
    return Plan("mul_bytes", n, [k, p], [("out32", want), ("status", st_want)],
                lambda eng, rt, i, out: eng.mul_bytes_dev(i[0], i[1], out[0], out[1], n, kind=algo), note=algo + (" undecodable" if kw.get("bad") else ""))


@kind("fixed", ("mul_endo_fixed", "mul_windowed_fixed"))
def _(d, n, st, rng, **kw):
    algo, base, off = opt(kw, "algo", rng, ("endo", "windowed")), opt(kw, "base", rng, ("G", "P2")), offset(kw, rng, n, d.rows)
    k, b = d.k[off:off + n], d.bases[base]
    table = b.te if algo == "endo" else b.tw
    want = oc.mul(oc.ENDO if algo == "endo" else oc.WINDOWED, k, None, table)
    return Plan("fixed", n, [k], [("out_r1", want)],
                lambda eng, rt, i, out: (eng.mul_endo_fixed_dev if algo == "endo" else eng.mul_windowed_fixed_dev)(i[0], table, out[0], n), note="%s table of %s" % (algo, base))


@kind("mixed", ("mul_endo_mixed",))
def _(d, n, st, rng, **kw):
    base, off = opt(kw, "base", rng, ("G", "P2")), offset(kw, rng, n, d.rows)
    k, p, f, table = d.k[off:off + n], d.p_r1[off:off + n], d.flags[off:off + n], d.bases[base].te
    want = np.where(f[:, None] == 0, oc.mul(oc.ENDO, k, None, table), d.var_r1[off:off + n])
    return Plan("mixed", n, [k, p, f], [("out_r1", want)], lambda eng, rt, i, out: eng.mul_endo_mixed_dev(i[0], i[1], i[2], table, out[0], n), note="table of %s" % base)


@kind("dh", ("dh_endo", "dh_windowed"))
def _(d, n, st, rng, **kw):
    algo = opt(kw, "algo", rng, ("endo", "windowed") if n <= 4099 else ("endo",))
    table392, off = opt(kw, "table392", rng, (None, "G", "P2")), offset(kw, rng, n, d.rows)
    k, p = d.k[off:off + n], d.p_aff[off:off + n]
    table = None
    if table392:
        b = d.bases[{"G": "G392", "P2": "P2x392"}[table392]]
        table = b.te if algo == "endo" else b.tw
    if algo == "endo" and table is None:
        want, wst = d.dh_var[off:off + n], zeros(n)
    else:
        want, wst = oc.dh(oc.ENDO if algo == "endo" else oc.WINDOWED, k, p, table)
    return Plan("dh", n, [k, p], [("out_affine", want), ("status", wst)],
                lambda eng, rt, i, out: (eng.dh_endo_dev if algo == "endo" else eng.dh_windowed_dev)(i[0], i[1], table, out[0], out[1], n),
                note="%s table392=%s" % (algo, table392))


@kind("dh_bytes", ("dh_endo_bytes", "dh_windowed_bytes"))
def _(d, n, st, rng, **kw):
    algo, off = opt(kw, "algo", rng, ("endo", "windowed")), offset(kw, rng, n, d.rows)
    k = d.k[off:off + n]
    if kw.get("bad"):
        enc, wst = refused_rows(RESTATED)
        keys, want, wst = enc[:n], np.zeros((n, 32), dtype=np.uint8), wst[:n]
    else:
        keys = d.p_enc[off:off + n]
        aff, wst = oc.dh(oc.ENDO if algo == "endo" else oc.WINDOWED, k, d.p_aff[off:off + n])
        want = np.ascontiguousarray(oc.encode(aff))
        assert not wst.any()
    return Plan("dh_bytes", n, [k, keys], [("out32", want), ("status", wst)],
                lambda eng, rt, i, out: eng.dh_bytes_dev(i[0], i[1], None, out[0], out[1], n, kind=algo), note=algo + (" undecodable" if kw.get("bad") else ""))


@kind("exchange", ("dh_exchange",))
def _(d, n, st, rng, **kw):
    base, with_table, off = opt(kw, "base", rng, ("G", "P2")), opt(kw, "with_table", rng, (False, True)), offset(kw, rng, n, d.rows)
    a, b = d.k[off:off + n], d.l[off:off + n]
    base_aff = d.bases[base].aff
    table = d.bases[{"G": "G392", "P2": "P2x392"}[base]].te if with_table else None
    mid, st1 = oc.dh(oc.ENDO, b, np.tile(base_aff, (n, 1)), table)
    want, st2 = oc.dh(oc.ENDO, a, mid)
    assert not st1.any() and not st2.any()
    return Plan("exchange", n, [a, b], [("out_affine", want), ("status", st2)],
                lambda eng, rt, i, out: eng.dh_exchange_dev(i[0], i[1], base_aff, table, out[0], out[1], n), note="base %s table392=%s" % (base, with_table))


@kind("exchange_comb", ("dh_exchange_comb",))
def _(d, n, st, rng, **kw):
    comb, b_, note = comb_of(d, st, kw, rng, ("G392", "P2x392", "G", "P2"))
    off = offset(kw, rng, n, d.rows)
    a, b = d.k[off:off + n], d.l[off:off + n]
    want, wst = oc.dh(oc.ENDO, a, oc.r1_to_affine(oc.mul(oc.ENDO, b, None, b_.te)))          # DH_endo(a_i, [b_i]B) for the comb's base B
    assert not wst.any()
    return Plan("exchange_comb", n, [a, b], [("out_affine", want), ("status", wst)],
                lambda eng, rt, i, out: eng.dh_exchange_comb_dev(i[0], i[1], comb, out[0], out[1], n), note=note)


@kind("comb_mul", ("comb_mul",))
def _(d, n, st, rng, **kw):
    comb, b_, note = comb_of(d, st, kw, rng, ("G", "P2", "G392", "P2x392"))
    off = offset(kw, rng, n, d.rows)
    k = d.k[off:off + n]
    want = oc.r1_to_affine(oc.mul(oc.ENDO, k, None, b_.te))
    if producer(kw, st, rng):
        less = k.copy()
        less[:, 0] -= np.uint64(1)
        one = np.zeros_like(k)
        one[:, 0] = 1

        def call(eng, rt, i, out):
            import torch
            with torch.cuda.stream(rt.side):
                i[0].add_(i[1])
            eng.comb_mul_dev(i[0], comb, out[0], out[1], n)
        return Plan("comb_mul", n, [less, one], [("out_affine", want), ("status", zeros(n))], call, note=note + " after a producer")
    return Plan("comb_mul", n, [k], [("out_affine", want), ("status", zeros(n))], lambda eng, rt, i, out: eng.comb_mul_dev(i[0], comb, out[0], out[1], n), note=note)


def double_sums(d, b_, off, n):
    """[k]B + [l][t]G = [(k c + l t) mod N]G for B = [c]G: canonical affine words and encodings"""
    aff = d.multiples_of_g([k * b_.c + l * t for k, l, t in zip(d.ki[off:off + n], d.li[off:off + n], d.ti[off:off + n])])
    return aff, np.ascontiguousarray(oc.encode(aff))


@kind("double_mul", ("double_mul_affine",))
def _(d, n, st, rng, **kw):
    comb, b_, note = comb_of(d, st, kw, rng)
    off = offset(kw, rng, n, d.rows)
    want, _ = double_sums(d, b_, off, n)
    return Plan("double_mul", n, [d.k[off:off + n], d.l[off:off + n], d.p_aff[off:off + n]], [("out_affine", want)],
                lambda eng, rt, i, out: eng.double_mul_dev(i[0], i[1], i[2], out[0], n, comb_host=comb), note=note)


@kind("double_mul_bytes", ("double_mul_bytes",))
def _(d, n, st, rng, **kw):
    comb, b_, note = comb_of(d, st, kw, rng)
    off = offset(kw, rng, n, d.rows)
    _, want = double_sums(d, b_, off, n)
    return Plan("double_mul_bytes", n, [d.k[off:off + n], d.l[off:off + n], d.p_enc[off:off + n]], [("out32", want), ("status", zeros(n))],
                lambda eng, rt, i, out: eng.double_mul_bytes_dev(i[0], i[1], i[2], out[0], out[1], n, comb_host=comb), note=note)


@kind("verify_bytes", ("verify_bytes",))
def _(d, n, st, rng, **kw):
    comb, b_, note = comb_of(d, st, kw, rng)
    off = offset(kw, rng, n, d.rows)
    _, expect = double_sums(d, b_, off, n)
    expect, ok = expect.copy(), np.ones(n, dtype=np.uint8)
    for i in {0, n // 2}:                            # two rows that must NOT verify
        expect[i, 7] ^= 4
        ok[i] = 0
    return Plan("verify_bytes", n, [d.k[off:off + n], d.l[off:off + n], d.p_enc[off:off + n], expect], [("ok", ok), ("status", zeros(n))],
                lambda eng, rt, i, out: eng.verify_bytes_dev(i[0], i[1], i[2], i[3], out[0], out[1], n, comb_host=comb), note=note)


def msm_shape(kw, rng, n):
    groups = opt(kw, "groups", rng, (1, n))
    return groups, n // groups


@kind("msm", ("msm_affine",))
def _(d, n, st, rng, **kw):
    (groups, size), off = msm_shape(kw, rng, n), offset(kw, rng, n, d.rows)
    want = d.multiples_of_g([sum(d.ki[off + g * size + j] * d.ti[off + g * size + j] for j in range(size)) for g in range(groups)])
    return Plan("msm", n, [d.k[off:off + n], d.p_aff[off:off + n]], [("out_affine", want)],
                lambda eng, rt, i, out: eng.msm_dev(i[0], i[1], out[0], groups, size), note="%d x %d" % (groups, size))


@kind("msm_bytes", ("msm_bytes",))
def _(d, n, st, rng, **kw):
    (groups, size), off = msm_shape(kw, rng, n), offset(kw, rng, n, d.rows)
    want = np.ascontiguousarray(oc.encode(d.multiples_of_g([sum(d.ki[off + g * size + j] * d.ti[off + g * size + j] for j in range(size)) for g in range(groups)])))
    enc, wst = d.p_enc[off:off + n].copy(), zeros(groups)
    if kw.get("bad"):                                # undecodable elements: their group reports 16 + the largest code and is zero
        bad, codes = refused_rows(RESTATED)
        for i in sorted({0, n // 3, n - 1}):
            enc[i] = bad[i % RESTATED]
            g = i // size
            wst[g] = max(wst[g], codes[i % RESTATED])
        want = want.copy()
        want[wst != 0] = 0
    return Plan("msm_bytes", n, [d.k[off:off + n], enc], [("out32", want), ("status", wst)],
                lambda eng, rt, i, out: eng.msm_bytes_dev(i[0], i[1], out[0], out[1], groups, size), note="%d x %d%s" % (groups, size, " undecodable" if kw.get("bad") else ""))


@kind("encode", ("encode",))
def _(d, n, st, rng, **kw):
    off = offset(kw, rng, n, d.rows)
    return Plan("encode", n, [d.p_aff[off:off + n]], [("out32", d.p_enc[off:off + n])], lambda eng, rt, i, out: eng.encode_dev(i[0], out[0], n))


@kind("decode", ("decode",))
def _(d, n, st, rng, **kw):
    off = offset(kw, rng, n, d.rows)
    return Plan("decode", n, [d.p_enc[off:off + n]], [("out_affine", d.p_aff[off:off + n]), ("status", zeros(n))], lambda eng, rt, i, out: eng.decode_dev(i[0], out[0], out[1], n))


@kind("sha512", ("sha512",))
def _(d, n, st, rng, **kw):
    m, lens, want = sha_batch()
    off = offset(kw, rng, n, len(m))
    return Plan("sha512", n, [m[off:off + n], lens[off:off + n]], [("out64", want[off:off + n])], lambda eng, rt, i, out: eng.sha512_dev(i[0], m.shape[1], i[1], 0, out[0], n))


def sig_comb(d, st, kw, rng):
    return comb_of(d, st, kw, rng, ("G",))


@kind("sig_keygen", ("sig_keygen",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    comb, _, note = sig_comb(d, st, kw, rng)
    c = sig_batch()
    return Plan("sig_keygen", n, [c["sk"][:n]], [("pk32", c["pk"][:n])], lambda eng, rt, i, out: eng.sig_keygen_dev(i[0], out[0], n, comb_host=comb), note=note)


@kind("sig_sign", ("sig_sign",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    comb, _, note = sig_comb(d, st, kw, rng)
    c = sig_batch()
    return Plan("sig_sign", n, [c["sk"][:n], c["pk"][:n], c["m"][:n], c["lens"][:n]], [("sig64", c["sig"][:n])],
                lambda eng, rt, i, out: eng.sig_sign_dev(i[0], i[1], i[2], c["m"].shape[1], i[3], 0, out[0], n, comb_host=comb), note=note)


@kind("sig_verify", ("sig_verify",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    comb, _, note = sig_comb(d, st, kw, rng)
    c = sig_batch()
    pk, sig, ok, wst = c["pk"][:n].copy(), c["sig"][:n].copy(), np.ones(n, dtype=np.uint8), zeros(n)
    if kw.get("bad"):                                # keys that do not decode on every third row
        for i in range(0, n, 3):
            pk[i] = refused_rows(RESTATED)[0][i]
            ok[i], wst[i] = sig_verdict(i, "key")
    for i in {n // 2, n - 1}:
        if wst[i] == 0:
            sig[i, 5] ^= 1
            ok[i], wst[i] = sig_verdict(i, "R")
    assert ok.sum() < n
    return Plan("sig_verify", n, [pk, c["m"][:n], c["lens"][:n], sig], [("ok", ok), ("status", wst)],
                lambda eng, rt, i, out: eng.sig_verify_dev(i[0], i[1], c["m"].shape[1], i[2], 0, i[3], out[0], out[1], n, comb_host=comb),
                note=note + (" undecodable keys" if kw.get("bad") else ""))


@kind("hash_to_field", ("hash_to_field",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    mode, c = opt(kw, "mode", rng, ("ro", "nu")), h2c_batch()
    return Plan("hash_to_field", n, [c["m"][:n], c["lens"][:n]], [("out_u", c["u_" + mode][:n])],
                lambda eng, rt, i, out: eng.hash_to_field_dev(i[0], c["m"].shape[1], i[1], 0, out[0], n, dst=c["dst"], mode=mode), note=mode)


@kind("map_to_curve", ("map_to_curve",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    c = h2c_batch()
    return Plan("map_to_curve", n, [c["u_nu"][:n]], [("out_affine", c["map"][:n])], lambda eng, rt, i, out: eng.map_to_curve_dev(i[0], out[0], n))


@kind("hash_to_curve", ("hash_to_curve", "hash_to_curve_affine"), cap=RESTATED)
def _(d, n, st, rng, **kw):
    mode, affine, c = opt(kw, "mode", rng, ("ro", "nu")), opt(kw, "affine", rng, (False, True)), h2c_batch()
    want = c[("aff_" if affine else "enc_") + mode][:n]
    return Plan("hash_to_curve", n, [c["m"][:n], c["lens"][:n]], [("out", want)],
                lambda eng, rt, i, out: eng.hash_to_curve_dev(i[0], c["m"].shape[1], i[1], 0, out[0], n, dst=c["dst"], mode=mode, affine=affine),
                note="%s %s" % (mode, "affine" if affine else "bytes"))


@kind("oprf_blind", ("oprf_blind",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    c = oprf_batch()
    return Plan("oprf_blind", n, [c["m160"][:n], c["lens"][:n], c["r"][:n]], [("out32", c["blinded"][:n]), ("status", zeros(n))],
                lambda eng, rt, i, out: eng.oprf_blind_dev(i[0], 160, i[1], 0, i[2], out[0], out[1], n, dst=c["dst"]))


@kind("oprf_evaluate", ("oprf_evaluate",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    c = oprf_batch()
    blinded, want, wst = c["blinded"][:n], c["evaluated"][:n], zeros(n)
    if kw.get("bad"):
        blinded = refused_rows(RESTATED)[0][:n]
        want, wst = (x[:n] for x in oprf_rejected(RESTATED)[2:])
    return Plan("oprf_evaluate", n, [blinded], [("out32", want), ("status", wst)], lambda eng, rt, i, out: eng.oprf_evaluate_dev(c["k"], i[0], out[0], out[1], n),
                note="undecodable" if kw.get("bad") else "")


@kind("oprf_finalize", ("oprf_finalize",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    c = oprf_batch()
    z, want, wst = c["evaluated"][:n], c["output"][:n], zeros(n)
    if kw.get("bad"):
        z = refused_rows(RESTATED)[0][:n]
        want, wst = (x[:n] for x in oprf_rejected(RESTATED)[:2])
    return Plan("oprf_finalize", n, [c["m160"][:n], c["lens"][:n], c["r"][:n], z], [("out64", want), ("status", wst)],
                lambda eng, rt, i, out: eng.oprf_finalize_dev(i[0], 160, i[1], 0, i[2], i[3], out[0], out[1], n, dst=c["dst"]), note="undecodable" if kw.get("bad") else "")


@kind("oprf_eval", ("oprf_eval",), cap=RESTATED)
def _(d, n, st, rng, **kw):
    c = oprf_batch()
    return Plan("oprf_eval", n, [c["m160"][:n], c["lens"][:n]], [("out64", c["output"][:n]), ("status", zeros(n))],
                lambda eng, rt, i, out: eng.oprf_eval_dev(c["k"], i[0], 160, i[1], 0, out[0], out[1], n, dst=c["dst"]))


@kind("scalar_inv", ("scalar_inv",))
def _(d, n, st, rng, **kw):
    off = offset(kw, rng, n, d.rows)
    want = codec.pack_scalars([pow(v % N, -1, N) if v % N else 0 for v in d.ki[off:off + n]])
    return Plan("scalar_inv", n, [d.k[off:off + n]], [("out", want)], lambda eng, rt, i, out: eng.scalar_inv_dev(i[0], out[0], n))


# ---- changes of the context's state, as steps of their own ------------------------------------------------------------------------------
@kind("comb_stage")
def _(d, n, st, rng, **kw):
    name = opt(kw, "comb", rng, ("G", "P2"))
    st.comb = name
    comb = d.bases[name].comb
    return Plan("comb_stage", 0, [], [], lambda eng, rt, i, out: eng.comb_stage(comb), note=name)


@kind("ct_flip")
def _(d, n, st, rng, **kw):
    def call(eng, rt, i, out):
        eng.ct_select = not eng.ct_select
    return Plan("ct_flip", 0, [], [], call)


@kind("set_stream")
def _(d, n, st, rng, **kw):
    st.side = kw["side"] if "side" in kw else not st.side
    side = st.side

    def call(eng, rt, i, out):                       # the header's contract: let the current stream's work finish, then hand over the other one
        eng.sync()
        eng.set_stream(rt.side.cuda_stream if side else None)
    return Plan("set_stream", 0, [], [], call, note="external" if side else "own")


@kind("tables_of_p3")
def _(d, n, st, rng, **kw):
    """fourq_comb_table and fourq_table_endo for a third point: kernels over scratch, comb_packed and table_packed that must leave what is
    staged alone (include/fourq_amd.h); they are host calls and return the oracle's tables"""
    b = d.bases["P3"]
    return Plan("tables_of_p3", 0, [], [], lambda eng, rt, i, out: [eng.comb_table(b.r1).reshape(-1, 12), eng.table_endo(b.r1).reshape(8, 16), eng.table_windowed(b.r1).reshape(8, 16)],
                host_wants=[("comb_table", b.comb.reshape(-1, 12)), ("table_endo", b.te.reshape(8, 16)), ("table_windowed", b.tw.reshape(8, 16))])


@kind("prim")
def _(d, n, st, rng, **kw):
    x, want = fp2_mul_rows(n)
    return Plan("prim", n, [], [], lambda eng, rt, i, out: [eng.prim("FP2_MUL", x)], host_wants=[("FP2_MUL", want)])


@kind("host_mul")
def _(d, n, st, rng, **kw):
    """a host-array call between _dev calls; rows past the pool repeat it"""
    reps = -(-n // d.rows)
    k, p, want = (np.tile(a, (reps, 1))[:n] for a in (d.k, d.p_r1, d.var_r1))

    def call(eng, rt, i, out):
        got = eng.mul_endo(k, p)
        rt.host_stats.append(eng.host_stats())
        return [got]
    return Plan("host_mul", n, [], [], call, host_wants=[("mul_endo", want)])


@kind("host_dh_bytes")
def _(d, n, st, rng, **kw):
    off = offset(kw, rng, n, d.rows)
    k, keys = d.k[off:off + n], d.p_enc[off:off + n]
    want = np.ascontiguousarray(oc.encode(d.dh_var[off:off + n]))

    def call(eng, rt, i, out):
        got = eng.dh_bytes(k, keys)
        rt.host_stats.append(eng.host_stats())
        return list(got)
    return Plan("host_dh_bytes", n, [], [], call, host_wants=[("out32", want), ("status", zeros(n))])


@kind("reserve")
def _(d, n, st, rng, **kw):
    return Plan("reserve", n, [], [], lambda eng, rt, i, out: eng.reserve(n))


STATE_KINDS = ("comb_stage", "ct_flip", "set_stream", "tables_of_p3", "prim", "host_mul", "host_dh_bytes", "reserve")
SIZES = (1, 7, 257, 4099)


@functools.lru_cache(maxsize=None)
def seeded_sequence(seed, steps=40):
    """`steps` plans: every third one a change of state, the others drawn from the _dev families, n from SIZES (restatement-backed kinds capped)"""
    rng = random.Random(seed)
    st = State()
    calls = [k for k in KINDS if k not in STATE_KINDS]
    plans = []
    for i in range(steps):
        if i % 3 == 2:
            name = rng.choice(STATE_KINDS)
            n = {"prim": rng.choice((64, 5000)), "host_mul": rng.choice((7, 2978)), "host_dh_bytes": 7, "reserve": rng.choice(SIZES)}.get(name, 0)
        else:
            name = rng.choice(calls)
            n = rng.choice([s for s in SIZES if KINDS[name].cap is None or s <= KINDS[name].cap])
        plans.append(build(name, n, st, rng))
    return tuple(plans)
