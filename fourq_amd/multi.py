"""All GPUs of a node behind ONE call: `MultiEngine` shards the rows of a host-array batch contiguously over one
`Engine` (one fourq_ctx, one HIP stream) per device and runs the shards side by side, one host thread per device.

SURVEY.md section 8(e): every (scalar, point) pair is independent, so there is no exchange step and no collective --
shard g owns rows [g*n/G, (g+1)*n/G) (`dist.shard_bounds`, the same cut the one-process-per-GPU path of bench.py and
`dist.sharded_map` use) and writes its results straight into its rows of the caller's output arrays.  ctypes drops the
GIL for the duration of a library call, so the per-device pipelines (H2D, kernels, D2H) really
overlap.  The reference's API is a plain function call (curve4q.py:188, :405, :464-468); this is the same call with
the node's GPUs behind it.  Fixed-base tables and comb tables are replicated (1 KiB / 13 KiB per device).
Threshold sharing (`Engine.shamir_*`) is NOT sharded: its arrays are party-major, so a contiguous cut of the rows is not a
contiguous cut of the arrays, and its batches are small beside the ladders'; call it on `engines[0]` or on an `Engine`.

    with MultiEngine() as eng:                 # every visible MI355X; MultiEngine([0, 0]) = two contexts on GPU 0
        out = eng.mul_endo(scalars, points)    # same arrays, same results as Engine.mul_endo
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .dist import shard_bounds
from .engine import Engine, _host, _out


def device_count():
    """Usable gfx950 devices as the library sees them (fourq_device_count); 0 without a GPU."""
    n = ctypes.c_int()
    _lib.check(_lib.load().fourq_device_count(ctypes.byref(n)))
    return n.value


class MultiEngine:
    def __init__(self, devices=None):
        if devices is None:
            devices = list(range(device_count()))
        devices = [int(d) for d in devices]
        if not devices:
            raise _lib.FourQError("fourq_amd: no usable gfx950 HIP device (MultiEngine needs at least one; there is no CPU fallback)")
        self.devices = devices
        self.engines = []
        try:
            for d in devices:
                self.engines.append(Engine(d))
        except Exception:
            self.close()
            raise
        self._pool = ThreadPoolExecutor(max_workers=len(devices), thread_name_prefix="fourq-dev")

    # ---- lifetime ---------------------------------------------------------------------------------------------
    def close(self):
        pool, self._pool = getattr(self, "_pool", None), None
        if pool is not None:
            pool.shutdown(wait=True)
        for e in getattr(self, "engines", []):
            e.close()
        self.engines = []

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def ct_select(self):
        return self.engines[0].ct_select

    @ct_select.setter
    def ct_select(self, on):
        for e in self.engines:
            e.ct_select = on

    @property
    def lanes(self):
        return sum(e.lanes for e in self.engines)

    def sync(self):
        for e in self.engines:
            e.sync()

    # ---- the sharding itself ----------------------------------------------------------------------------------
    def _sharded(self, call, rows, outs):
        """`call(engine, *row_shards, *out_shards)` on every device's contiguous shard of the row arrays `rows`, results
        landing in the matching rows of `outs`.  Errors of any shard are raised after all shards have finished."""
        n = len(rows[0])
        world = len(self.engines)

        def one(g):
            lo, hi = shard_bounds(n, g, world)
            if hi > lo:
                call(self.engines[g], *[a[lo:hi] for a in rows], *[o[lo:hi] for o in outs])

        if world == 1 or n < 2:
            for g in range(world):
                one(g)
        else:
            for f in [self._pool.submit(one, g) for g in range(world)]:
                f.result()
        return outs[0] if len(outs) == 1 else tuple(outs)

    @staticmethod
    def _same_len(*arrays):
        if len({len(a) for a in arrays}) != 1:
            raise ValueError("row arrays differ in length")

    # ---- tables (device 0; tables are data, identical on every device) --------------------------------------------
    def table_endo(self, p_r1):
        return self.engines[0].table_endo(p_r1)

    def table_windowed(self, p_r1):
        return self.engines[0].table_windowed(p_r1)

    def comb_table(self, p_r1):
        return self.engines[0].comb_table(p_r1)

    # ---- scalar multiplication ------------------------------------------------------------------------------------
    def mul_endo(self, scalars, points_r1, out=None):
        s, p = _host(scalars, 4), _host(points_r1, 20)
        self._same_len(s, p)
        return self._sharded(lambda e, s, p, o: e.mul_endo(s, p, out=o), [s, p], [_out(out, len(s), 20)])

    def mul_windowed(self, scalars, points_r1, out=None):
        s, p = _host(scalars, 4), _host(points_r1, 20)
        self._same_len(s, p)
        return self._sharded(lambda e, s, p, o: e.mul_windowed(s, p, out=o), [s, p], [_out(out, len(s), 20)])

    def mul_endo_fixed(self, scalars, table, out=None):
        s = _host(scalars, 4)
        return self._sharded(lambda e, s, o: e.mul_endo_fixed(s, table, out=o), [s], [_out(out, len(s), 20)])

    def mul_windowed_fixed(self, scalars, table, out=None):
        s = _host(scalars, 4)
        return self._sharded(lambda e, s, o: e.mul_windowed_fixed(s, table, out=o), [s], [_out(out, len(s), 20)])

    def mul_endo_mixed(self, scalars, points_r1, flags, table, out=None):
        s, p, f = _host(scalars, 4), _host(points_r1, 20), _host(flags, None, np.uint8).ravel()
        self._same_len(s, p, f)
        return self._sharded(lambda e, s, p, f, o: e.mul_endo_mixed(s, p, f, table, out=o), [s, p, f], [_out(out, len(s), 20)])

    # ---- Diffie-Hellman -------------------------------------------------------------------------------------------
    def dh_endo(self, scalars, points_affine, table=None, out=None, status=None):
        s, p = _host(scalars, 4), _host(points_affine, 8)
        self._same_len(s, p)
        return self._sharded(lambda e, s, p, o, st: e.dh_endo(s, p, table, out=o, status=st), [s, p],
                             [_out(out, len(s), 8), _out(status, len(s), None, np.uint8)])

    def dh_windowed(self, scalars, points_affine, table=None, out=None, status=None):
        s, p = _host(scalars, 4), _host(points_affine, 8)
        self._same_len(s, p)
        return self._sharded(lambda e, s, p, o, st: e.dh_windowed(s, p, table, out=o, status=st), [s, p],
                             [_out(out, len(s), 8), _out(status, len(s), None, np.uint8)])

    def dh_exchange(self, a_scalars, b_scalars, base_affine, table392=None, out=None, status=None):
        a, b = _host(a_scalars, 4), _host(b_scalars, 4)
        self._same_len(a, b)
        return self._sharded(lambda e, a, b, o, st: e.dh_exchange(a, b, base_affine, table392, out=o, status=st), [a, b],
                             [_out(out, len(a), 8), _out(status, len(a), None, np.uint8)])

    def dh_exchange_comb(self, a_scalars, b_scalars, comb, out=None, status=None):
        a, b = _host(a_scalars, 4), _host(b_scalars, 4)
        self._same_len(a, b)
        return self._sharded(lambda e, a, b, o, st: e.dh_exchange_comb(a, b, comb, out=o, status=st), [a, b],
                             [_out(out, len(a), 8), _out(status, len(a), None, np.uint8)])

    def comb_mul(self, scalars, comb, out=None, status=None):
        s = _host(scalars, 4)
        return self._sharded(lambda e, s, o, st: e.comb_mul(s, comb, out=o, status=st), [s],
                             [_out(out, len(s), 8), _out(status, len(s), None, np.uint8)])

    # ---- [k]B + [l]P and signature checks -------------------------------------------------------------------------
    def double_mul(self, k_scalars, l_scalars, points_affine, comb, out=None):
        k, l, p = _host(k_scalars, 4), _host(l_scalars, 4), _host(points_affine, 8)
        self._same_len(k, l, p)
        return self._sharded(lambda e, k, l, p, o: e.double_mul(k, l, p, comb, out=o), [k, l, p], [_out(out, len(k), 8)])

    def verify_bytes(self, k_scalars, l_scalars, keys32, expect32, comb, ok=None, status=None):
        k, l = _host(k_scalars, 4), _host(l_scalars, 4)
        a, x = _host(keys32, 32, np.uint8), _host(expect32, 32, np.uint8)
        self._same_len(k, l, a, x)
        return self._sharded(lambda e, k, l, a, x, o, st: e.verify_bytes(k, l, a, x, comb, ok=o, status=st), [k, l, a, x],
                             [_out(ok, len(k), None, np.uint8), _out(status, len(k), None, np.uint8)])

    def sig_sign(self, sk32, pk32, msgs, lens=None, comb=None, out=None):
        sk, pk, m = _host(sk32, 32, np.uint8), _host(pk32, 32, np.uint8), np.ascontiguousarray(msgs, dtype=np.uint8)
        ln = np.full(len(m), m.shape[1], dtype=np.uint32) if lens is None else np.ascontiguousarray(lens, dtype=np.uint32).ravel()
        self._same_len(sk, pk, m, ln)
        return self._sharded(lambda e, sk, pk, m, ln, o: e.sig_sign(sk, pk, m, ln, comb, out=o), [sk, pk, m, ln], [_out(out, len(sk), 64, np.uint8)])

    def sig_verify(self, pk32, msgs, sig64, lens=None, comb=None, ok=None, status=None):
        pk, sig, m = _host(pk32, 32, np.uint8), _host(sig64, 64, np.uint8), np.ascontiguousarray(msgs, dtype=np.uint8)
        ln = np.full(len(m), m.shape[1], dtype=np.uint32) if lens is None else np.ascontiguousarray(lens, dtype=np.uint32).ravel()
        self._same_len(pk, sig, m, ln)
        return self._sharded(lambda e, pk, m, sig, ln, o, st: e.sig_verify(pk, m, sig, ln, comb, ok=o, status=st), [pk, m, sig, ln],
                             [_out(ok, len(pk), None, np.uint8), _out(status, len(pk), None, np.uint8)])

    # ---- signatures of registered keys: the set is replicated on every device, rows are sharded --------------------------------------
    def keyset_set(self, keys32):
        pk = _host(keys32, 32, np.uint8)
        status = None
        for e in self.engines:
            status = e.keyset_set(pk)
        return status

    def keyset_count(self):
        return self.engines[0].keyset_count()

    def keyset_reserve(self, n):
        for e in self.engines:
            e.keyset_reserve(n)

    def keyset_double_mul_bytes(self, k_scalars, l_scalars, ids, comb=None, out=None, status=None):
        k, l, i = _host(k_scalars, 4), _host(l_scalars, 4), np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        self._same_len(k, l, i)
        return self._sharded(lambda e, k, l, i, o, st: e.keyset_double_mul_bytes(k, l, i, comb, out=o, status=st), [k, l, i],
                             [_out(out, len(k), 32, np.uint8), _out(status, len(k), None, np.uint8)])

    def sig_verify_keyed(self, ids, msgs, sig64, lens=None, comb=None, ok=None, status=None):
        i, sig, m = np.ascontiguousarray(ids, dtype=np.uint32).ravel(), _host(sig64, 64, np.uint8), np.ascontiguousarray(msgs, dtype=np.uint8)
        ln = np.full(len(m), m.shape[1], dtype=np.uint32) if lens is None else np.ascontiguousarray(lens, dtype=np.uint32).ravel()
        self._same_len(i, sig, m, ln)
        return self._sharded(lambda e, i, m, sig, ln, o, st: e.sig_verify_keyed(i, m, sig, ln, comb, ok=o, status=st), [i, m, sig, ln],
                             [_out(ok, len(i), None, np.uint8), _out(status, len(i), None, np.uint8)])

    def hash_to_curve(self, msgs, lens=None, dst=b"", mode="ro", affine=False, out=None):
        m = np.ascontiguousarray(msgs, dtype=np.uint8)
        ln = np.full(len(m), m.shape[1], dtype=np.uint32) if lens is None else np.ascontiguousarray(lens, dtype=np.uint32).ravel()
        self._same_len(m, ln)
        out = _out(out, len(m), 8) if affine else _out(out, len(m), 32, np.uint8)
        return self._sharded(lambda e, m, ln, o: e.hash_to_curve(m, ln, dst, mode, affine, out=o), [m, ln], [out])

    # ---- oblivious PRF: rows are independent, the key and dst are replicated ------------------------------------------
    @staticmethod
    def _msg_rows(msgs, lens):
        m = np.ascontiguousarray(msgs, dtype=np.uint8)
        ln = np.full(len(m), m.shape[1], dtype=np.uint32) if lens is None else np.ascontiguousarray(lens, dtype=np.uint32).ravel()
        return m, ln

    def oprf_blind(self, msgs, blinds, lens=None, dst=b"", out=None, status=None):
        (m, ln), r = self._msg_rows(msgs, lens), _host(blinds, 4)
        self._same_len(m, ln, r)
        return self._sharded(lambda e, m, ln, r, o, st: e.oprf_blind(m, r, ln, dst, out=o, status=st), [m, ln, r],
                             [_out(out, len(r), 32, np.uint8), _out(status, len(r), None, np.uint8)])

    def oprf_evaluate(self, key, blinded32, out=None, status=None):
        b = _host(blinded32, 32, np.uint8)
        return self._sharded(lambda e, b, o, st: e.oprf_evaluate(key, b, out=o, status=st), [b],
                             [_out(out, len(b), 32, np.uint8), _out(status, len(b), None, np.uint8)])

    def oprf_finalize(self, msgs, blinds, evaluated32, lens=None, dst=b"", out=None, status=None):
        (m, ln), r, z = self._msg_rows(msgs, lens), _host(blinds, 4), _host(evaluated32, 32, np.uint8)
        self._same_len(m, ln, r, z)
        return self._sharded(lambda e, m, ln, r, z, o, st: e.oprf_finalize(m, r, z, ln, dst, out=o, status=st), [m, ln, r, z],
                             [_out(out, len(r), 64, np.uint8), _out(status, len(r), None, np.uint8)])

    def oprf_eval(self, key, msgs, lens=None, dst=b"", out=None, status=None):
        m, ln = self._msg_rows(msgs, lens)
        self._same_len(m, ln)
        return self._sharded(lambda e, m, ln, o, st: e.oprf_eval(key, m, ln, dst, out=o, status=st), [m, ln],
                             [_out(out, len(m), 64, np.uint8), _out(status, len(m), None, np.uint8)])

    # ---- oblivious PRF: proofs.  A proof covers a whole group, so WHOLE groups are sharded: device g owns the groups shard_bounds gives it
    # and, with them, their rows ----------------------------------------------------------------------------------------------------------
    def _sharded_groups(self, call, rows, per_group, outs, group_size):
        """as _sharded, cut between groups: `rows` have group_size rows per group, `per_group` and `outs` one"""
        groups, world = len(outs[0]), len(self.engines)

        def one(g):
            lo, hi = shard_bounds(groups, g, world)
            if hi > lo:
                call(self.engines[g], *[a[lo * group_size:hi * group_size] for a in rows], *[a[lo:hi] for a in per_group], *[o[lo:hi] for o in outs])

        if world == 1 or groups < 2:
            for g in range(world):
                one(g)
        else:
            for f in [self._pool.submit(one, g) for g in range(world)]:
                f.result()
        return tuple(outs)

    def dleq_public_key(self, key):
        return self.engines[0].dleq_public_key(key)

    def dleq_prove(self, key, blinded32, evaluated32, nonces, group_size=None, dst=b"", comb=None, out=None, status=None):
        b, z, r = _host(blinded32, 32, np.uint8), _host(evaluated32, 32, np.uint8), _host(nonces, 4)
        self._same_len(b, z)
        groups, group_size = Engine._groups(len(b), max(len(b), 1) if group_size is None else group_size)
        if len(r) != groups:
            raise ValueError("one nonce per group")
        return self._sharded_groups(lambda e, b, z, r, o, st: e.dleq_prove(key, b, z, r, group_size, dst, comb, out=o, status=st), [b, z], [r],
                                    [_out(out, groups, 64, np.uint8), _out(status, groups, None, np.uint8)], group_size)

    def dleq_verify(self, pk32, blinded32, evaluated32, proofs64, group_size=None, dst=b"", comb=None, ok=None, status=None):
        b, z, p = _host(blinded32, 32, np.uint8), _host(evaluated32, 32, np.uint8), _host(proofs64, 64, np.uint8)
        self._same_len(b, z)
        groups, group_size = Engine._groups(len(b), max(len(b), 1) if group_size is None else group_size)
        if len(p) != groups:
            raise ValueError("one proof per group")
        return self._sharded_groups(lambda e, b, z, p, o, st: e.dleq_verify(pk32, b, z, p, group_size, dst, comb, ok=o, status=st), [b, z], [p],
                                    [_out(ok, groups, None, np.uint8), _out(status, groups, None, np.uint8)], group_size)

    # ---- verifiable random function: rows are independent; dst, and for the keyed call the set, are replicated -----------------------------
    def vrf_prove(self, sk32, pk32, alphas, lens=None, dst=b"", comb=None, out=None):
        sk, pk, (m, ln) = _host(sk32, 32, np.uint8), _host(pk32, 32, np.uint8), self._msg_rows(alphas, lens)
        self._same_len(sk, pk, m, ln)
        return self._sharded(lambda e, sk, pk, m, ln, o: e.vrf_prove(sk, pk, m, ln, dst, comb, out=o), [sk, pk, m, ln], [_out(out, len(sk), 96, np.uint8)])

    def vrf_verify(self, pk32, alphas, proofs96, lens=None, dst=b"", comb=None, beta=None, ok=None, status=None):
        pk, p, (m, ln) = _host(pk32, 32, np.uint8), _host(proofs96, 96, np.uint8), self._msg_rows(alphas, lens)
        self._same_len(pk, p, m, ln)
        return self._sharded(lambda e, pk, m, p, ln, b, o, st: e.vrf_verify(pk, m, p, ln, dst, comb, beta=b, ok=o, status=st), [pk, m, p, ln],
                             [_out(beta, len(pk), 64, np.uint8), _out(ok, len(pk), None, np.uint8), _out(status, len(pk), None, np.uint8)])

    def vrf_verify_keyed(self, ids, alphas, proofs96, lens=None, dst=b"", comb=None, beta=None, ok=None, status=None):
        i, p, (m, ln) = np.ascontiguousarray(ids, dtype=np.uint32).ravel(), _host(proofs96, 96, np.uint8), self._msg_rows(alphas, lens)
        self._same_len(i, p, m, ln)
        return self._sharded(lambda e, i, m, p, ln, b, o, st: e.vrf_verify_keyed(i, m, p, ln, dst, comb, beta=b, ok=o, status=st), [i, m, p, ln],
                             [_out(beta, len(i), 64, np.uint8), _out(ok, len(i), None, np.uint8), _out(status, len(i), None, np.uint8)])

    def vrf_proof_to_hash(self, proofs96, dst=b"", beta=None, status=None):
        p = _host(proofs96, 96, np.uint8)
        return self._sharded(lambda e, p, b, st: e.vrf_proof_to_hash(p, dst, beta=b, status=st), [p],
                             [_out(beta, len(p), 64, np.uint8), _out(status, len(p), None, np.uint8)])

    # ---- commitments over a fixed generator set: the set is replicated, WHOLE groups are sharded as for the proofs -----------------------
    def commit_generators(self, count, dst):
        return self.engines[0].commit_generators(count, dst)

    def commit_bases(self, points_affine):
        p = _host(points_affine, 8)
        for e in self.engines:
            e.commit_bases(p)

    @property
    def commit_bases_count(self):
        return self.engines[0].commit_bases_count

    def commit(self, scalars, group_size, route=0, out=None):
        k = _host(scalars, 4)
        groups, group_size = Engine._groups(len(k), group_size)
        return self._sharded_groups(lambda e, k, o: e.commit(k, group_size, route, out=o), [k], [], [_out(out, groups, 8)], group_size)[0]

    def commit_bytes(self, scalars, group_size, route=0, out=None):
        k = _host(scalars, 4)
        groups, group_size = Engine._groups(len(k), group_size)
        return self._sharded_groups(lambda e, k, o: e.commit_bytes(k, group_size, route, out=o), [k], [], [_out(out, groups, 32, np.uint8)], group_size)[0]

    # ---- wire format ----------------------------------------------------------------------------------------------
    def encode(self, points_affine, out=None):
        p = _host(points_affine, 8)
        return self._sharded(lambda e, p, o: e.encode(p, out=o), [p], [_out(out, len(p), 32, np.uint8)])

    def decode(self, encodings, out=None, status=None):
        b = _host(encodings, 32, np.uint8)
        return self._sharded(lambda e, b, o, st: e.decode(b, out=o, status=st), [b],
                             [_out(out, len(b), 8), _out(status, len(b), None, np.uint8)])

    def dh_bytes(self, scalars, public_keys32, kind="endo", table=None, out=None, status=None):
        s, k = _host(scalars, 4), _host(public_keys32, 32, np.uint8)
        self._same_len(s, k)
        return self._sharded(lambda e, s, k, o, st: e.dh_bytes(s, k, kind, table, out=o, status=st), [s, k],
                             [_out(out, len(s), 32, np.uint8), _out(status, len(s), None, np.uint8)])


__all__ = ["MultiEngine", "device_count"]
