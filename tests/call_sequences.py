"""Helper of tests/test_gpu_call_sequences.py: a table of step kinds -- one per family of `_dev` entry points, plus the changes of a
context's state -- each of which builds a Plan: the host arrays of one call, the expected bytes of every output, and the call itself.
A run uploads every plan's inputs, allocates every output pre-filled with 0xA5, enqueues the calls with nothing in between, synchronises
the engine ONCE and compares.

Expected values never come from the library: the C oracle (oracle/oracle_c.py) with the modular arithmetic in Python integers -- group-law
identities such as [k]B + [l][t]G = [(k c + l t) mod N]G for B = [c]G -- hashlib, pow, and the restatements tests/sig_ref.py, tests/h2c_ref.py
and tests/oprf_ref.py through the cached seeded batches of their GPU test modules.  Tables and combs are the oracle's too (data only).
Everything is computed once per process and shared by all engines and both selection modes.

The later families -- registered keys, commitments, ragged and bucket sums, DLEQ, the VRF, threshold sharing -- have kinds of their own
below the first table: the grouped sums by the group law sum [k_i][t_i]G = [(sum k_i t_i) mod N]G (commitments over bases [c_j]G with known
c_j), the others by tests/keyset_ref.py, dleq_ref.py, vrf_ref.py and shamir_ref.py, each with a refused, spoiled or tampered row among honest
ones.  The key set, the commitment bases and the ragged shape are objects the context holds: State records which one is installed, a
call that needs another installs it in front of itself, and state kinds replace them between calls in flight.  check_entry_points and
check_state_calls compare the table with the binding: every `_dev` name, and every name that sets or reserves something on a context."""
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
ENTRY = "fourq_%s%s"                  # % (a kind's entry, its suffix): the first families end in _batch_dev, the later ones in _dev


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
    """What the builders need to know of the context's history to say what a call must return: which comb `comb == NULL` means, and which
    key set, commitment bases and ragged shape the context holds (names of KEYSETS, BASE_SETS and SHAPES); the inversion group is recorded
    only -- it changes no byte."""

    def __init__(self):
        self.comb = None
        self.side = False
        self.keyset = self.bases = self.shape = None
        self.scinv = 0


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
    def __init__(self, name, entries, cap, build, sets=()):
        self.name, self.entries, self.cap, self.build, self.sets = name, entries, cap, build, sets


def kind(name, entries=(), cap=None, suffix="_batch_dev", sets=()):
    """entries: the _dev entry points the kind calls, without "fourq_" and the suffix; sets: the calls that set or reserve something on a
    context which the kind stands for, by their full names"""
    def deco(fn):
        KINDS[name] = Kind(name, tuple(ENTRY % (e, suffix) for e in entries), cap, fn, tuple(sets))
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
        enc, st_want = refused_rows(max(n, RESTATED))
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
@kind("comb_stage", sets=("fourq_comb_stage",))
def _(d, n, st, rng, **kw):
    name = opt(kw, "comb", rng, ("G", "P2"))
    st.comb = name
    comb = d.bases[name].comb
    return Plan("comb_stage", 0, [], [], lambda eng, rt, i, out: eng.comb_stage(comb), note=name)


@kind("ct_flip", sets=("fourq_ctx_set_ct_select",))
def _(d, n, st, rng, **kw):
    def call(eng, rt, i, out):
        eng.ct_select = not eng.ct_select
    return Plan("ct_flip", 0, [], [], call)


@kind("set_stream", sets=("fourq_ctx_set_stream",))
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


@kind("reserve", sets=("fourq_ctx_reserve",))
def _(d, n, st, rng, **kw):
    return Plan("reserve", n, [], [], lambda eng, rt, i, out: eng.reserve(n))


FIRST_KINDS = tuple(KINDS)           # the table as the first three seeds drew from it: frozen, so that their sequences never change
FIRST_STATE_KINDS = ("comb_stage", "ct_flip", "set_stream", "tables_of_p3", "prim", "host_mul", "host_dh_bytes", "reserve")


# ---- the later families: objects the context holds, grouped sums, keyed calls, DLEQ, the VRF, threshold sharing ---------------------------
GROUP_SIZES = (1, 7, 65)             # 65: one past the 64-row fold team, and past one 64-row part of a bucket
SHAPES = {"one": (0, 1, 0), "seven": (0, 1, 0, 5, 1, 0), "small": (0, 1, 0, 30, 1, 1, 0), "mid": (0, 65, 1, 0, 126, 65, 0), "wide": (0, 2000, 65, 0, 1, 1, 2032, 0)}      # group lengths
KEYSETS = {"A": (5, None), "B": (16, 2)}                           # name -> (keys, the slot whose key does not decode)
KEYED_ROWS = {"A": 65, "B": RESTATED}                              # the rows restated over each set: calls over A stay at 65
BASE_SETS = {"A": 8, "B": 65}
DLEQ_SHAPES = ((1, 1), (3, 11), (5, 51))
SHAMIR_T = (1, 3, 5)


def shape_rows(name):
    return sum(SHAPES[name])


def rows_of(items, width):
    return np.frombuffer(b"".join(bytes(b) for b in items), dtype=np.uint8).reshape(len(items), width).copy()


@functools.lru_cache(maxsize=None)
def keyset(name):
    """a key set over the signature batch's keys: the registered bytes, the batch row that owns each slot (None: refused), and the statuses
    fourq_keyset_set must return, by tests/keyset_ref.py"""
    import keyset_ref
    m, refused = KEYSETS[name]
    first = {"A": 0, "B": 8}[name]
    keys = sig_batch()["pk"][first:first + m].copy()
    owner = list(range(first, first + m))
    if refused is not None:
        keys[refused], owner[refused] = refused_rows(RESTATED)[0][1], None
    status = np.array([keyset_ref.key_status(k.tobytes()) for k in keys], dtype=np.uint8)
    assert [s != 0 for s in status] == [row is None for row in owner]
    return {"keys": keys, "bytes": [k.tobytes() for k in keys], "owner": owner, "status": status}


@functools.lru_cache(maxsize=None)
def keyed_ids(name):
    """RESTATED ids over the set, random, with every slot in turn from row 8; rows 0 and 5 (the one whose proof is spoiled) name accepted
    keys, row 1 the refused slot (where the set has one), row 3 one past the set"""
    m, refused = KEYSETS[name]
    ids = np.random.default_rng(9110 + m).integers(0, m, size=KEYED_ROWS[name]).astype(np.uint32)
    ids[8:8 + m] = np.arange(m)
    ids[0], ids[5] = 0, m - 1
    if refused is not None:
        ids[1] = refused
    ids[3] = m
    return ids


def signer_of(ks, key_id):
    """the batch row whose secret key signs for a row that names `key_id`; rows that are refused anyway are signed by the set's first key"""
    owner = ks["owner"][key_id] if key_id < len(ks["owner"]) else None
    return ks["owner"][0] if owner is None else owner


@functools.lru_cache(maxsize=None)
def keyed_sig_rows(name):
    """signatures of the batch's messages under the keys the ids name, row 5 spoiled; (ids, sigs, ok, status) by the restatements"""
    import keyset_ref
    import sig_ref
    c, ks, ids = sig_batch(), keyset(name), keyed_ids(name)
    sks = [c["sk"][signer_of(ks, int(i))].tobytes() for i in ids]
    pks = [c["pk"][signer_of(ks, int(i))].tobytes() for i in ids]
    sigs = sig_ref.batch_sign(sks, pks, c["msgs"][:len(ids)]).copy()
    sigs[5, 5] ^= 1
    verdicts = [keyset_ref.verify_keyed(ks["bytes"], int(i), msg, s.tobytes()) for i, msg, s in zip(ids, c["msgs"], sigs)]
    ok, status = (np.array([v[j] for v in verdicts], dtype=np.uint8) for j in (0, 1))
    assert status[3] == keyset_ref.KEYSET_ID_RANGE and not ok[5] and not status[5] and ok[0]
    return ids, sigs, ok, status


@functools.lru_cache(maxsize=None)
def keyed_double_rows(name):
    """[k]G + [l]A_id over the pool's first scalars: (ids, out32, status) by tests/keyset_ref.py"""
    import keyset_ref
    d, ks, ids = data(4099), keyset(name), keyed_ids(name)
    rows = [keyset_ref.double_mul_keyed(ks["bytes"], int(i), k, l) for i, k, l in zip(ids, d.ki, d.li)]
    return ids, rows_of([r[0] for r in rows], 32), np.array([r[1] for r in rows], dtype=np.uint8)


def keyset_of(st, kw, rng):
    """(the set's name, whether the call has to install it first): the installed one unless another is asked for"""
    name = kw.get("keyset") or st.keyset or rng.choice(sorted(KEYSETS))
    install, st.keyset = name != st.keyset, name
    return name, install


def install_keyset(eng, name):
    """fourq_keyset_set of the set; what it returns is compared with the restatement's slot statuses as a host result of the step"""
    return eng.keyset_set(keyset(name)["keys"])


@kind("keyed_double_mul", ("keyset_double_mul_bytes",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    comb, _, note = sig_comb(d, st, kw, rng)
    name, install = keyset_of(st, kw, rng)
    ids, want, wst = keyed_double_rows(name)
    n = min(n, len(ids))

    def call(eng, rt, i, out):
        host = [install_keyset(eng, name)] if install else []
        eng.keyset_double_mul_bytes_dev(i[0], i[1], i[2], out[0], out[1], n, comb_host=comb)
        return host
    return Plan("keyed_double_mul", n, [d.k[:n], d.l[:n], ids[:n]], [("out32", want[:n]), ("status", wst[:n])], call,
                host_wants=[("key_status", keyset(name)["status"])] if install else (), note="%s keys %s%s" % (note, name, " installed here" if install else ""))


@kind("keyed_verify", ("keyset_sig_verify",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    comb, _, note = sig_comb(d, st, kw, rng)
    name, install = keyset_of(st, kw, rng)
    c = sig_batch()
    ids, sigs, ok, wst = keyed_sig_rows(name)
    n = min(n, len(ids))

    def call(eng, rt, i, out):
        host = [install_keyset(eng, name)] if install else []
        eng.sig_verify_keyed_dev(i[0], i[1], c["m"].shape[1], i[2], 0, i[3], out[0], out[1], n, comb_host=comb)
        return host
    return Plan("keyed_verify", n, [ids[:n], c["m"][:n], c["lens"][:n], sigs[:n]], [("ok", ok[:n]), ("status", wst[:n])], call,
                host_wants=[("key_status", keyset(name)["status"])] if install else (), note="%s keys %s%s" % (note, name, " installed here" if install else ""))


# ---- grouped sums by the group law: ragged, bucket route, commitments ----------------------------------------------------------------------
def group_sums(d, index_groups, coeff=None):
    """canonical affine words of [(sum over the group of k_i c_i) mod N]G, c_i = t_i of the pool's points unless `coeff` gives it"""
    return d.multiples_of_g([sum(d.ki[i] * (d.ti[i] if coeff is None else coeff(i)) for i in idx) for idx in index_groups])


def spoiled_rows(d, off, n, index_groups, want_enc):
    """the bytes flavour with three rows that do not decode: their groups report 16 + the largest code and are zero"""
    enc, wst, want = d.p_enc[off:off + n].copy(), zeros(len(index_groups)), want_enc.copy()
    bad, codes = refused_rows(RESTATED)
    group_of = {i: g for g, idx in enumerate(index_groups) for i in idx}
    for i in sorted({0, n // 3, n - 1}):
        enc[i] = bad[i % RESTATED]
        wst[group_of[off + i]] = max(wst[group_of[off + i]], codes[i % RESTATED])
    want[wst != 0] = 0
    return enc, want, wst


def grouped_shape(kw, rng, n, most_groups=None):
    size = opt(kw, "size", rng, [s for s in GROUP_SIZES if s <= n])
    groups = kw.get("groups") or max(1, n // size)
    return (min(groups, most_groups) if most_groups else groups), size


def shape_of(st, kw, rng, n):
    """(the shape's name, whether the call installs it first): the installed one unless another is asked for; none installed: the largest
    of at most n rows"""
    name = kw.get("shape") or st.shape or max((s for s in SHAPES if shape_rows(s) <= max(n, 1)), key=shape_rows)
    install, st.shape = name != st.shape, name
    return name, install


def offsets_of(name):
    return np.concatenate([[0], np.cumsum(SHAPES[name])]).astype(np.uint32)


@kind("ragged", ("raggedsum_affine", "raggedsum_bytes"), suffix="_dev")
def _(d, n, st, rng, **kw):
    flavour = opt(kw, "flavour", rng, ("affine", "bytes"))
    name, install = shape_of(st, kw, rng, n)
    offs = offsets_of(name)
    rows, off = int(offs[-1]), 0
    idx = [range(off + int(a), off + int(b)) for a, b in zip(offs[:-1], offs[1:])]
    want = group_sums(d, idx)
    ins, wants = [d.k[off:off + rows], d.p_aff[off:off + rows]], [("out_affine", want)]
    if flavour == "bytes":
        enc, want32, wst = d.p_enc[off:off + rows], np.ascontiguousarray(oc.encode(want)), zeros(len(idx))
        if kw.get("bad"):
            enc, want32, wst = spoiled_rows(d, off, rows, idx, want32)
        ins, wants = [d.k[off:off + rows], enc], [("out32", want32), ("status", wst)]

    def call(eng, rt, i, out):
        if install:
            eng.msm_shape(offs)
        (eng.msm_ragged_dev if flavour == "affine" else eng.msm_ragged_bytes_dev)(i[0], i[1], *out)
    return Plan("ragged", rows, ins, wants, call, note="%s shape %s%s%s" % (flavour, name, " installed here" if install else "", " undecodable" if kw.get("bad") else ""))


@kind("bucket", ("bucketsum_affine", "bucketsum_bytes"), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    """an explicit window: window 0 takes the ladder route at these sizes.  At most 33 groups -- a group's buckets take a quarter of a
    megabyte of the work buffer"""
    flavour, window = opt(kw, "flavour", rng, ("affine", "bytes")), opt(kw, "window", rng, (4, 5))
    groups, size = grouped_shape(kw, rng, n, most_groups=33)
    rows = groups * size
    off = offset(kw, rng, rows, d.rows)
    idx = [range(off + g * size, off + (g + 1) * size) for g in range(groups)]
    want = group_sums(d, idx)
    note = "%s %d x %d window %d" % (flavour, groups, size, window)
    if flavour == "affine":
        return Plan("bucket", rows, [d.k[off:off + rows], d.p_aff[off:off + rows]], [("out_affine", want)],
                    lambda eng, rt, i, out: eng.bucket_sum_dev(i[0], i[1], out[0], groups, size, window), note=note)
    enc, want32, wst = d.p_enc[off:off + rows], np.ascontiguousarray(oc.encode(want)), zeros(groups)
    if kw.get("bad"):
        enc, want32, wst = spoiled_rows(d, off, rows, idx, want32)
    return Plan("bucket", rows, [d.k[off:off + rows], enc], [("out32", want32), ("status", wst)],
                lambda eng, rt, i, out: eng.bucket_sum_bytes_dev(i[0], i[1], out[0], out[1], groups, size, window), note=note + (" undecodable" if kw.get("bad") else ""))


@functools.lru_cache(maxsize=None)
def base_set(name):
    """BASE_SETS[name] bases [c_j]G with known c_j: (the c_j, their canonical affine words)"""
    rng = random.Random(9120 + BASE_SETS[name])
    cs = [rng.randrange(1, N) for _ in range(BASE_SETS[name])]
    return cs, data(4099).multiples_of_g(cs)


def bases_of(st, kw, rng, size=0):
    """(the set's name, whether the call installs it first): the installed one unless another is asked for or it has too few bases"""
    fits = [s for s in sorted(BASE_SETS) if BASE_SETS[s] >= size]
    name = kw.get("bases") or (st.bases if st.bases in fits else rng.choice(fits))
    install, st.bases = name != st.bases, name
    return name, install


@kind("commit", ("commit_affine", "commit_bytes"), suffix="_dev")
def _(d, n, st, rng, **kw):
    flavour, route = opt(kw, "flavour", rng, ("affine", "bytes")), opt(kw, "route", rng, (1, 2, 0))
    groups, size = grouped_shape(kw, rng, n)
    name, install = bases_of(st, kw, rng, size)
    cs, aff = base_set(name)
    rows = groups * size
    off = offset(kw, rng, rows, d.rows)
    want = group_sums(d, [range(off + g * size, off + (g + 1) * size) for g in range(groups)], coeff=lambda i: cs[(i - off) % size])
    if flavour == "bytes":
        want = np.ascontiguousarray(oc.encode(want))

    def call(eng, rt, i, out):
        if install:
            eng.commit_bases(aff)
        (eng.commit_dev if flavour == "affine" else eng.commit_bytes_dev)(i[0], out[0], groups, size, route)
    return Plan("commit", rows, [d.k[off:off + rows]], [("out", want)], call,
                note="%s %d x %d route %d bases %s%s" % (flavour, groups, size, route, name, " installed here" if install else ""))


# ---- DLEQ: tests/dleq_ref.py through the cached shapes of tests/test_gpu_dleq.py ---------------------------------------------------------
def dleq_shape(kw, rng, n):
    return kw.get("dleq") or rng.choice([s for s in DLEQ_SHAPES if s[0] * s[1] <= n])


@functools.lru_cache(maxsize=None)
def dleq_verdicts(groups, size):
    """the shape's honest rows with two evaluated rows of group 1 exchanged (where there is a group 1): (evaluated, ok, status) by the
    restatement -- one tampered group among honest ones"""
    import dleq_ref
    import test_gpu_dleq as t
    s = t.shape(groups, size)
    e = s["e"].copy()
    if groups > 1 and size > 1:
        e[[size, size + 1]] = e[[size + 1, size]]
    v = dleq_ref.verify(s["pk"], s["b"], e, s["proofs"], t.DST, size)
    ok, status = (np.array([x[j] for x in v], dtype=np.uint8) for j in (0, 1))
    assert not status.any() and ok.tolist() == [0 if (g == 1 and size > 1) else 1 for g in range(groups)]
    return e, ok, status


@kind("dleq_composites", ("dleq_composites",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    import test_gpu_dleq as t
    groups, size = dleq_shape(kw, rng, n)
    s = t.shape(groups, size)
    return Plan("dleq_composites", groups * size, [s["b"], s["e"]], [("M32", s["m32"]), ("Z32", s["z32"]), ("status", zeros(groups))],
                lambda eng, rt, i, out: eng.dleq_composites_dev(s["pk"], i[0], i[1], out[0], out[1], out[2], groups, size, dst=t.DST), note="%d x %d" % (groups, size))


@kind("dleq_prove", ("dleq_prove",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    import test_gpu_dleq as t
    comb, _, note = sig_comb(d, st, kw, rng)
    groups, size = dleq_shape(kw, rng, n)
    s = t.shape(groups, size)
    return Plan("dleq_prove", groups * size, [s["b"], s["e"], s["r"]], [("proof64", s["proofs"]), ("status", zeros(groups))],
                lambda eng, rt, i, out: eng.dleq_prove_dev(s["k"], i[0], i[1], i[2], out[0], out[1], groups, size, dst=t.DST, comb_host=comb),
                note="%d x %d %s" % (groups, size, note))


@kind("dleq_verify", ("dleq_verify",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    import test_gpu_dleq as t
    comb, _, note = sig_comb(d, st, kw, rng)
    groups, size = dleq_shape(kw, rng, n)
    s = t.shape(groups, size)
    e, ok, wst = dleq_verdicts(groups, size)
    return Plan("dleq_verify", groups * size, [s["b"], e, s["proofs"]], [("ok", ok), ("status", wst)],
                lambda eng, rt, i, out: eng.dleq_verify_dev(s["pk"], i[0], i[1], i[2], out[0], out[1], groups, size, dst=t.DST, comb_host=comb),
                note="%d x %d %s" % (groups, size, note))


# ---- the VRF: tests/vrf_ref.py through the cached batch of tests/test_gpu_vrf.py -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vrf_rows():
    """the batch with row 2's proof spoiled (a bit of s) and row 4's key one that does not decode: keys, proofs and (beta, ok, status) by
    the restatement; proof_to_hash with row 6's Gamma one that does not decode"""
    import test_gpu_vrf as t
    import vrf_ref
    b = t.batch()
    pks, proofs = b["pks"].copy(), b["proofs"].copy()
    proofs[2, 64] ^= 1
    pks[4] = refused_rows(RESTATED)[0][4]
    v = [vrf_ref.verify(pk.tobytes(), a, p.tobytes(), t.DST) for pk, a, p in zip(pks, b["alphas"], proofs)]
    want = (rows_of([x[2] for x in v], 64), np.array([x[0] for x in v], dtype=np.uint8), np.array([x[1] for x in v], dtype=np.uint8))
    assert want[1].sum() == t.ROWS - 2 and want[2][4] and not want[2][2] and np.array_equal(want[0][want[1] == 1], b["betas"][want[1] == 1])
    gammas = b["proofs"].copy()
    gammas[6, :32] = refused_rows(RESTATED)[0][7]
    h = [vrf_ref.proof_to_hash(p.tobytes(), t.DST) for p in gammas]
    assert h[6][1] and not h[5][1]
    return {"pks": pks, "proofs": proofs, "want": want, "gammas": gammas, "hash": (rows_of([x[0] for x in h], 64), np.array([x[1] for x in h], dtype=np.uint8))}


@functools.lru_cache(maxsize=None)
def vrf_keyed_rows(name):
    """proofs of the batch's alphas under the keys the ids name, row 5 spoiled: (ids, proofs, (beta, ok, status)) by the restatement"""
    import test_gpu_vrf as t
    import vrf_ref
    c, b, ks, ids = sig_batch(), t.batch(), keyset(name), keyed_ids(name)
    own = [signer_of(ks, int(i)) for i in ids]
    proofs = rows_of([vrf_ref.prove(c["sk"][j].tobytes(), c["pk"][j].tobytes(), a, t.DST) for j, a in zip(own, b["alphas"])], 96)
    proofs[5, 64] ^= 1
    v = [vrf_ref.verify_keyed(ks["bytes"], int(i), a, p.tobytes(), t.DST) for i, a, p in zip(ids, b["alphas"], proofs)]
    want = (rows_of([x[2] for x in v], 64), np.array([x[0] for x in v], dtype=np.uint8), np.array([x[1] for x in v], dtype=np.uint8))
    assert want[1][0] and not want[1][5] and not want[2][5] and want[2][3] == _lib.KEYSET_ID_RANGE
    return ids, proofs, want


@kind("vrf_prove", ("vrf_prove",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    import test_gpu_vrf as t
    comb, _, note = sig_comb(d, st, kw, rng)
    b = t.batch()
    return Plan("vrf_prove", n, [b["sks"][:n], b["pks"][:n], b["matrix"][:n], b["lens"][:n]], [("proof96", b["proofs"][:n])],
                lambda eng, rt, i, out: eng.vrf_prove_dev(i[0], i[1], i[2], t.STRIDE, i[3], 0, out[0], n, dst=t.DST, comb_host=comb), note=note)


@kind("vrf_verify", ("vrf_verify",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    import test_gpu_vrf as t
    comb, _, note = sig_comb(d, st, kw, rng)
    b, r = t.batch(), vrf_rows()
    return Plan("vrf_verify", n, [r["pks"][:n], b["matrix"][:n], b["lens"][:n], r["proofs"][:n]], [(label, w[:n]) for label, w in zip(("beta64", "ok", "status"), r["want"])],
                lambda eng, rt, i, out: eng.vrf_verify_dev(i[0], i[1], t.STRIDE, i[2], 0, i[3], out[0], out[1], out[2], n, dst=t.DST, comb_host=comb), note=note)


@kind("vrf_verify_keyed", ("vrf_verify_keyed",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    import test_gpu_vrf as t
    comb, _, note = sig_comb(d, st, kw, rng)
    name, install = keyset_of(st, kw, rng)
    b = t.batch()
    ids, proofs, want = vrf_keyed_rows(name)
    n = min(n, len(ids))

    def call(eng, rt, i, out):
        host = [install_keyset(eng, name)] if install else []
        eng.vrf_verify_keyed_dev(i[0], i[1], t.STRIDE, i[2], 0, i[3], out[0], out[1], out[2], n, dst=t.DST, comb_host=comb)
        return host
    return Plan("vrf_verify_keyed", n, [ids[:n], b["matrix"][:n], b["lens"][:n], proofs[:n]], [(label, w[:n]) for label, w in zip(("beta64", "ok", "status"), want)], call,
                host_wants=[("key_status", keyset(name)["status"])] if install else (), note="%s keys %s%s" % (note, name, " installed here" if install else ""))


@kind("vrf_proof_to_hash", ("vrf_proof_to_hash",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    import test_gpu_vrf as t
    r = vrf_rows()
    return Plan("vrf_proof_to_hash", n, [r["gammas"][:n]], [("beta64", r["hash"][0][:n]), ("status", r["hash"][1][:n])],
                lambda eng, rt, i, out: eng.vrf_proof_to_hash_dev(i[0], out[0], out[1], n, dst=t.DST))


# ---- threshold sharing: tests/shamir_ref.py ---------------------------------------------------------------------------------------------
PARTIES = (3, 1, 0xFFFFFFFF, 9, 4)


def shamir_shape(kw, rng, n):
    """(rows, t): t from SHAMIR_T, rows x t <= min(n, RESTATED) items"""
    t = opt(kw, "t", rng, [t for t in SHAMIR_T if t <= n])
    return max(1, min(n, RESTATED) // t), t


@functools.lru_cache(maxsize=None)
def shamir_dealt(rows, t):
    """`rows` polynomials of t coefficients below N (never 0, so that every commitment decodes), their commitments, one recipient per
    row and its share, by the restatement; row 1's share is wrong"""
    import shamir_ref
    rng = random.Random(9130 + 10 * rows + t)
    ps = [[rng.randrange(1, N) for _ in range(t)] for _ in range(rows)]
    ids = [rng.choice(PARTIES + (7, 1 << 31)) for _ in range(rows)]
    commits = rows_of([c for p in ps for c in shamir_ref.commitments(p)], 32).reshape(rows, t, 32)
    shares = [shamir_ref.horner(p, x) for p, x in zip(ps, ids)]
    if rows > 1:
        shares[1] = (shares[1] + 1) % N
    pub = [shamir_ref.public_share([bytes(c) for c in commits[g]], ids[g]) for g in range(rows)]
    ver = [shamir_ref.verify([bytes(c) for c in commits[g]], ids[g], shares[g]) for g in range(rows)]
    assert [v[0] for v in ver] == [0 if (g == 1) else 1 for g in range(rows)] and not any(v[1] for v in ver)
    return {"polys": ps, "ids": np.array(ids, dtype=np.uint32), "commits": commits, "shares": codec.pack_scalars(shares),
            "pub32": rows_of([x[0] for x in pub], 32), "pub_st": np.array([x[1] for x in pub], dtype=np.uint8),
            "ok": np.array([v[0] for v in ver], dtype=np.uint8), "ver_st": np.array([v[1] for v in ver], dtype=np.uint8)}


@functools.lru_cache(maxsize=None)
def shamir_values(rows, t, m):
    """shares of test_gpu_shamir's polynomials (edge values in every position) for the first m parties, party-major, by the restatement"""
    import shamir_ref
    from test_gpu_shamir import polys
    ps = polys(rows, t)
    blocks, status = shamir_ref.shares(ps, PARTIES[:m])
    return codec.pack_scalars([a for p in ps for a in p]), codec.pack_scalars([v for block in blocks for v in block]), np.array(status, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def shamir_sets(sets, t):
    """`sets` id sets of t distinct non-zero ids -- set 1 with its first id repeated, where t allows it -- and lambda by the restatement"""
    import shamir_ref
    rng = random.Random(9140 + 10 * sets + t)
    ids = [rng.sample(range(1, 1 << 32), t) for _ in range(sets)]
    if sets > 1 and t > 1:
        ids[1][t - 1] = ids[1][0]
    lam = [shamir_ref.lagrange(x) for x in ids]
    assert sets < 2 or t < 2 or (lam[1][1] == shamir_ref.ID_REPEATED and not any(lam[1][0]))
    return np.array(ids, dtype=np.uint32), codec.pack_scalars([v for l, _ in lam for v in l]), np.array([s for _, s in lam], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def shamir_combined(rows, t, repeated):
    """t blocks of `rows` shares and of `rows` encoded points (the pool's first), one id set: combine and combine_points by the restatement"""
    import shamir_ref
    d = data(4099)
    ids = list(PARTIES[:t])
    if repeated:
        ids[t - 1] = ids[0]
    blocks = [d.ki[i * rows:(i + 1) * rows] for i in range(t)]
    out, st = shamir_ref.combine(ids, blocks)
    pts = d.p_enc[:t * rows].reshape(t, rows, 32).copy()
    if rows > 2:
        pts[t - 1, 2] = refused_rows(RESTATED)[0][2]
    out32, st32 = shamir_ref.combine_points(ids, [[bytes(r) for r in block] for block in pts])
    return {"ids": np.array(ids, dtype=np.uint32), "shares": d.k[:t * rows], "out": codec.pack_scalars([0] * rows if st else out), "st": np.array([st], dtype=np.uint8),
            "pts": pts, "out32": rows_of(out32, 32), "st32": np.array(st32, dtype=np.uint8)}


@kind("shamir_shares", ("shamir_shares",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    (rows, t), m = shamir_shape(kw, rng, n), opt(kw, "m", rng, (1, 5))
    coeffs, shares, wst = shamir_values(rows, t, m)
    ids = np.array(PARTIES[:m], dtype=np.uint32)
    return Plan("shamir_shares", rows * t, [coeffs, ids], [("shares", shares), ("status", wst)],
                lambda eng, rt, i, out: eng.shamir_shares_dev(i[0], i[1], out[0], out[1], rows, t, m), note="%d x %d for %d parties" % (rows, t, m))


@kind("shamir_lagrange", ("shamir_lagrange",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    sets, t = shamir_shape(kw, rng, n)
    ids, lam, wst = shamir_sets(sets, t)
    return Plan("shamir_lagrange", sets * t, [ids], [("lambda", lam), ("status", wst)], lambda eng, rt, i, out: eng.shamir_lagrange_dev(i[0], out[0], out[1], sets, t),
                note="%d sets of %d" % (sets, t))


@kind("shamir_combine", ("shamir_combine",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    rows, t = shamir_shape(kw, rng, n)
    c = shamir_combined(rows, t, bool(kw.get("bad")) and t > 1)
    return Plan("shamir_combine", rows * t, [c["ids"], c["shares"]], [("out", c["out"]), ("status", c["st"])],
                lambda eng, rt, i, out: eng.shamir_combine_dev(i[0], i[1], out[0], out[1], rows, t), note="%d x %d%s" % (rows, t, " repeated id" if kw.get("bad") else ""))


@kind("shamir_combine_points", ("shamir_combine_points",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    rows, t = shamir_shape(kw, rng, n)
    c = shamir_combined(rows, t, bool(kw.get("bad")) and t > 1)
    return Plan("shamir_combine_points", rows * t, [c["ids"], c["pts"]], [("out32", c["out32"]), ("status", c["st32"])],
                lambda eng, rt, i, out: eng.shamir_combine_points_dev(i[0], i[1], out[0], out[1], rows, t), note="%d x %d%s" % (rows, t, " repeated id" if kw.get("bad") else ""))


@kind("shamir_public_shares", ("shamir_public_shares",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    rows, t = shamir_shape(kw, rng, n)
    c = shamir_dealt(rows, t)
    return Plan("shamir_public_shares", rows * t, [c["commits"], c["ids"]], [("out32", c["pub32"]), ("status", c["pub_st"])],
                lambda eng, rt, i, out: eng.shamir_public_shares_dev(i[0], i[1], out[0], out[1], rows, t), note="%d x %d" % (rows, t))


@kind("shamir_verify", ("shamir_verify",), cap=RESTATED, suffix="_dev")
def _(d, n, st, rng, **kw):
    comb, _, note = sig_comb(d, st, kw, rng)
    rows, t = shamir_shape(kw, rng, n)
    c = shamir_dealt(rows, t)
    return Plan("shamir_verify", rows * t, [c["commits"], c["ids"], c["shares"]], [("ok", c["ok"]), ("status", c["ver_st"])],
                lambda eng, rt, i, out: eng.shamir_verify_dev(i[0], i[1], i[2], out[0], out[1], rows, t, comb_host=comb), note="%d x %d %s" % (rows, t, note))


# ---- the later families' objects and reservations, as steps of their own: synchronous host calls between calls in flight ----------------
@kind("keyset_set", sets=("fourq_keyset_set",))
def _(d, n, st, rng, **kw):
    name = st.keyset = opt(kw, "keyset", rng, sorted(KEYSETS))
    return Plan("keyset_set", 0, [], [], lambda eng, rt, i, out: [eng.keyset_set(keyset(name)["keys"])], host_wants=[("key_status", keyset(name)["status"])], note=name)


@kind("commit_bases", sets=("fourq_commit_bases_set",))
def _(d, n, st, rng, **kw):
    name = st.bases = opt(kw, "bases", rng, sorted(BASE_SETS))
    aff = base_set(name)[1]
    return Plan("commit_bases", 0, [], [], lambda eng, rt, i, out: eng.commit_bases(aff), note=name)


@kind("msm_shape", sets=("fourq_raggedsum_shape_set",))
def _(d, n, st, rng, **kw):
    name = st.shape = opt(kw, "shape", rng, sorted(SHAPES))
    offs = offsets_of(name)
    return Plan("msm_shape", 0, [], [], lambda eng, rt, i, out: eng.msm_shape(offs), note=name)


@kind("scinv_group", sets=("fourq_ctx_set_scinv_group",))
def _(d, n, st, rng, **kw):
    k = st.scinv = opt(kw, "k", rng, (0, 1, 8, 16))
    return Plan("scinv_group", 0, [], [], lambda eng, rt, i, out: eng.set_scinv_group(k), note=str(k))


FAMILY_RESERVES = ("fourq_keyset_reserve", "fourq_commit_reserve", "fourq_bucketsum_reserve", "fourq_raggedsum_shape_reserve", "fourq_dleq_reserve", "fourq_vrf_reserve",
                   "fourq_shamir_reserve")


@kind("family_reserve", sets=FAMILY_RESERVES)
def _(d, n, st, rng, **kw):
    """every family's own reservation for n rows (the ragged one for the installed shape, where there is one)"""
    size = max(s for s in GROUP_SIZES if s <= max(n, 1))
    groups, shaped = max(1, n // size), st.shape is not None

    def call(eng, rt, i, out):
        eng.keyset_reserve(n)
        eng.commit_reserve(groups, size)
        eng.bucket_sum_reserve(min(groups, 33), size, 4)
        if shaped:
            eng.msm_shape_reserve()
        eng.dleq_reserve(groups, size)
        eng.vrf_reserve(n)
        eng.shamir_reserve(max(1, n // 5), 5)
    return Plan("family_reserve", n, [], [], call, note="%d x %d" % (groups, size))


@kind("host_keyed")
def _(d, n, st, rng, **kw):
    """one host-array call each of the later families between _dev calls: commit_bytes, msm_ragged_bytes, sig_verify_keyed and
    shamir_combine_points; each installs what it needs where it is not installed"""
    which = opt(kw, "which", rng, ("commit_bytes", "msm_ragged_bytes", "sig_verify_keyed", "shamir_combine_points"))
    if which == "commit_bytes":
        groups, size = grouped_shape(kw, rng, n)
        name, _ = bases_of(st, kw, rng, size)
        cs, aff = base_set(name)
        want = np.ascontiguousarray(oc.encode(group_sums(d, [range(g * size, (g + 1) * size) for g in range(groups)], coeff=lambda i: cs[i % size])))
        call, wants = (lambda eng: [eng.commit_bases(aff), eng.commit_bytes(d.k[:groups * size], size)][1:]), [("out32", want)]
    elif which == "msm_ragged_bytes":
        name = st.shape = kw.get("shape") or max((s for s in SHAPES if shape_rows(s) <= max(n, 1)), key=shape_rows)
        offs = offsets_of(name)
        rows = int(offs[-1])
        want = np.ascontiguousarray(oc.encode(group_sums(d, [range(int(a), int(b)) for a, b in zip(offs[:-1], offs[1:])])))
        call, wants = (lambda eng: list(eng.msm_ragged_bytes(d.k[:rows], d.p_enc[:rows], offs))), [("out32", want), ("status", zeros(len(offs) - 1))]
    elif which == "sig_verify_keyed":
        name = st.keyset = kw.get("keyset") or st.keyset or "A"
        c, n = sig_batch(), min(n, KEYED_ROWS[name])
        ids, sigs, ok, wst = (x.copy() for x in keyed_sig_rows(name))
        if n > 3:                                    # the host flavour refuses an index outside the set: row 3 names the first key here, whose owner signed it
            import keyset_ref
            ids[3] = 0
            ok[3], wst[3] = keyset_ref.verify_keyed(keyset(name)["bytes"], 0, c["msgs"][3], sigs[3].tobytes())
        call = lambda eng: [eng.keyset_set(keyset(name)["keys"])] + list(eng.sig_verify_keyed(ids[:n], c["m"][:n], sigs[:n], c["lens"][:n], d.bases["G"].comb))
        wants = [("key_status", keyset(name)["status"]), ("ok", ok[:n]), ("status", wst[:n])]
        st.comb = "G"
    else:
        rows, t = shamir_shape(kw, rng, n)
        c = shamir_combined(rows, t, False)
        call, wants = (lambda eng: list(eng.shamir_combine_points(c["ids"], c["pts"]))), [("out32", c["out32"]), ("status", c["st32"])]

    def run_it(eng, rt, i, out):
        got = call(eng)
        rt.host_stats.append(eng.host_stats())
        return got
    return Plan("host_keyed", n, [], [], run_it, host_wants=wants, note=which)


@functools.lru_cache(maxsize=None)
def restated():
    """every restatement-backed expectation of the later families, computed here once per process instead of inside whichever test asks first"""
    for name in KEYSETS:
        keyed_sig_rows(name), keyed_double_rows(name), vrf_keyed_rows(name)
    vrf_rows()
    for groups, size in DLEQ_SHAPES:
        dleq_verdicts(groups, size)
    for t in SHAMIR_T:
        rows = RESTATED // t
        shamir_dealt(rows, t), shamir_combined(rows, t, False), shamir_sets(rows, t)
    return True


STATE_KINDS = FIRST_STATE_KINDS + ("keyset_set", "commit_bases", "msm_shape", "scinv_group", "family_reserve", "host_keyed")
# calls that set or reserve something on a context and are named by no kind, each with its reason
EXEMPT_STATE_CALLS = {"fourq_ctx_set_host_timing": "switches event records around the chunk copies of host-array calls on; no byte of any result depends on it"}
SIZES = (1, 7, 257, 4099)


def state_calls():
    """every name of the binding that sets or reserves something on a context"""
    import re
    return {name for name in _lib.PROTOTYPES if re.search(r"(_set|_reserve|_stage)$|_ctx_set_", name)}


def check_entry_points():
    """the table names every `_dev` entry point of the binding, whatever its suffix, and nothing else"""
    named = {e for k in KINDS.values() for e in k.entries}
    declared = {name for name in _lib.PROTOTYPES if name.endswith("_dev")}
    batch = {name for name in declared if name.endswith("_batch_dev")}
    assert len(batch) >= 36, sorted(batch)
    assert named == declared, (sorted(declared - named), sorted(named - declared))
    assert set(STATE_KINDS) == {name for name, k in KINDS.items() if not k.entries}


def check_state_calls():
    """every call that sets or reserves something on a context is named by a state kind, or exempt with a reason"""
    named = {s for name in STATE_KINDS for s in KINDS[name].sets}
    declared = state_calls()
    listed = {"fourq_keyset_set", "fourq_commit_bases_set", "fourq_raggedsum_shape_set", "fourq_ctx_set_scinv_group", "fourq_ctx_set_ct_select", "fourq_ctx_set_stream",
              "fourq_comb_stage", "fourq_ctx_reserve"} | set(FAMILY_RESERVES)
    assert listed <= declared and not named & set(EXEMPT_STATE_CALLS)
    assert named | set(EXEMPT_STATE_CALLS) == declared, (sorted(declared - named - set(EXEMPT_STATE_CALLS)), sorted((named | set(EXEMPT_STATE_CALLS)) - declared))
    assert all(not k.sets for name, k in KINDS.items() if name not in STATE_KINDS)


# ---- the later layouts behind dirt (tests/test_gpu_call_sequences.py, section 9): (kind, options, the layout it carves and its shape) ------
DIRT_ROWS = 4099                     # mul_bytes at this size rewrites rows_in and rows_out: bytes [0, 320 x 4099) of the work buffer, full R1 rows
DIRT_SUCCESSORS = [
    ("keyed_verify", {"keyset": "B"}, ("Keyset", 257)),
    ("commit", {"size": 1, "route": 1, "bases": "A", "flavour": "bytes"}, ("Commit", 257, 1)),
    ("commit", {"size": 65, "route": 2, "bases": "B", "flavour": "affine"}, ("Commit", 3, 65)),
    ("bucket", {"size": 257, "groups": 1, "window": 4, "flavour": "bytes"}, ("Bucket", 1, 257, 4)),
    ("bucket", {"size": 65, "window": 4, "flavour": "affine"}, ("Bucket", 3, 65, 4)),
    ("ragged", {"shape": "mid", "flavour": "bytes"}, ("MsmRagged", 257, 7)),
    ("dleq_verify", {"dleq": (5, 51)}, ("Dleq", 255, 5)),
    ("vrf_verify_keyed", {"keyset": "B"}, ("Vrf", 257)),
    ("shamir_verify", {"t": 5}, ("Shamir", 51, 5)),
    ("shamir_combine_points", {"t": 5}, ("Shamir", 51, 5)),
]
# the later families with rejected rows, for the reverse pair
DIRT_REJECTING = [("keyed_verify", {"keyset": "B"}), ("bucket", {"size": 65, "window": 4, "flavour": "bytes", "bad": True}), ("ragged", {"shape": "mid", "flavour": "bytes", "bad": True}),
                  ("dleq_verify", {"dleq": (5, 51)}), ("vrf_verify_keyed", {"keyset": "B"}), ("vrf_verify", {}), ("shamir_verify", {"t": 5}),
                  ("shamir_combine_points", {"t": 5, "bad": True}), ("commit", {"size": 7, "route": 0, "bases": "A", "flavour": "bytes"})]


@functools.lru_cache(maxsize=None)
def seeded_sequence(seed, steps=40, whole=False):
    """`steps` plans: every third one a change of state, the others drawn from the _dev families, n from SIZES (restatement-backed kinds capped).
    whole=False draws from the table as it was when the first three seeds were chosen (FIRST_KINDS), whole=True from all of it."""
    rng = random.Random(seed)
    st = State()
    states = STATE_KINDS if whole else FIRST_STATE_KINDS
    calls = [k for k in (KINDS if whole else FIRST_KINDS) if k not in states]
    plans = []
    for i in range(steps):
        if i % 3 == 2:
            name = rng.choice(states)
            n = {"prim": rng.choice((64, 5000)), "host_mul": rng.choice((7, 2978)), "host_dh_bytes": 7, "reserve": rng.choice(SIZES)}.get(name, 0)
            if name in ("family_reserve", "host_keyed"):
                n = rng.choice((7, 257))
        else:
            name = rng.choice(calls)
            n = rng.choice([s for s in SIZES if KINDS[name].cap is None or s <= KINDS[name].cap])
        plans.append(build(name, n, st, rng))
    return tuple(plans)
